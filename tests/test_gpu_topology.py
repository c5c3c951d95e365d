"""Mesh topology on the GPU: against the twin (integers equal, areas and volumes bit for bit), against tests/topology_reference.py, from
run to run, and on the meshes that spread one component over every XCD of the chip: where a stale parent would show."""
import numpy as np
import pytest
import torch

import topology_cases as K
import topology_reference as R
from shapegan_amd import metrics, topology as T
from shapegan_amd.mesh import MeshBatch, marching_cubes
from test_gpu_mesh import mixed_batch
from test_mesh import sphere_grid

pytestmark = pytest.mark.gpu

FIELDS = ("vertex_component", "comp_offsets", "shape_index", "vertices", "triangles", "edges", "open_edges", "area", "volume")


def to_cpu(batch):
    return MeshBatch(batch.vertices.cpu(), batch.normals.cpu(), batch.faces.cpu(), batch.vert_offsets.cpu(), batch.tri_offsets.cpu())


def assert_same_components(gpu, cpu):
    """Every field equal; area and volume (float64) bit for bit."""
    for k in FIELDS:
        a, b = getattr(gpu, k).cpu(), getattr(cpu, k)
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b), k


def check_against_twin(batch, rules=("largest", True)):
    """components and every keep rule on the device equal the twin's on the same mesh -> (device components, twin components)."""
    host = to_cpu(batch)
    gpu, cpu = T.components(batch), T.components(host)
    assert gpu.area.is_cuda and gpu.vertex_component.is_cuda
    assert_same_components(gpu, cpu)
    for rule in rules:
        mask_gpu, mask_cpu = T.select(gpu, rule), T.select(cpu, rule)
        assert torch.equal(mask_gpu.cpu(), mask_cpu)
        kept = T.keep_components(batch, gpu, mask_gpu)
        assert kept.vertices.is_cuda and K.same_batches(kept, T.keep_components(host, cpu, mask_cpu))
    return gpu, cpu


@pytest.mark.parametrize("seed,empties", [(0, False), (1, True)])
def test_mixed_batch_equals_the_twin_and_repeats(seed, empties):
    grids = mixed_batch(24, 32, seed)
    if empties:
        grids[[0, 11, 12, 23]] = 1.0      # no surface: empty shapes first, in the middle (two in a row) and last
    batch = marching_cubes(grids.cuda(), spacing=2 / 32, origin=-1)
    gpu, _ = check_against_twin(batch, rules=("largest", True, {"largest": 3, "min_triangles": 6, "drop_cavities": True}))
    assert len(gpu) > 1000
    if empties:
        assert gpu.counts()[[0, 11, 12, 23]].tolist() == [0, 0, 0, 0]
    again = T.components(batch)
    assert_same_components(again, type("C", (), {k: getattr(gpu, k).cpu() for k in FIELDS}))
    assert K.same_batches(batch.clean(True), batch.clean(True))


def test_small_batches_against_the_reference():
    grids = mixed_batch(6, 16, 4)
    grids[3] = 1.0
    for batch in (marching_cubes(grids.cuda(), spacing=2 / 16, origin=-1), K.hand_batch("cuda")[1]):
        comps, ref = T.components(batch), R.components(batch)
        R.check_against(comps, ref)
        for rule in ("largest", True, {"largest": 2, "min_triangles": 5}):
            mask = T.select(comps, rule)
            assert mask.tolist() == R.select(ref, rule).tolist()
            assert K.equals_reference(T.keep_components(batch, comps, mask), R.compact(batch, ref, mask.cpu().numpy()))


# ---- one component across every XCD ---------------------------------------------------------------------------------------------------
def reference_labels(batch):
    faces, vo, to = batch.faces.cpu().numpy(), batch.vert_offsets.tolist(), batch.tri_offsets.tolist()
    return np.concatenate([R.label_shape(faces[to[s]:to[s + 1]], vo[s + 1] - vo[s])[0] for s in range(len(vo) - 1)])


@pytest.fixture(scope="module")
def big_sphere():
    """One 128^3 sphere of radius 0.9 on the device, its components there and in the twin."""
    batch = K.mesh_grids(sphere_grid(128, 0.9)[None], "cuda")
    gpu, cpu = check_against_twin(batch)
    return batch, gpu, cpu


def test_big_sphere_is_one_component(big_sphere):
    batch, gpu, _ = big_sphere
    assert len(gpu) == 1 and gpu.triangles.item() > 100000 and gpu.watertight.item() and gpu.genus.item() == 0
    assert (gpu.vertex_component == 0).all()
    assert np.array_equal(gpu.vertex_component.cpu().numpy(), reference_labels(batch))
    assert K.same_batches(T.keep_components(batch, gpu, torch.ones(1)), batch)
    assert T.keep_components(batch, gpu, torch.zeros(1)).faces.shape[0] == 0


def test_permuted_big_sphere(big_sphere):
    batch, plain, _ = big_sphere
    shuffled, perm = K.permuted(batch, 5)
    gpu, _ = check_against_twin(shuffled)
    labels = gpu.vertex_component.cpu().numpy()
    assert np.array_equal(labels, reference_labels(shuffled))
    assert R.same_partition(labels[perm.cpu().numpy()], plain.vertex_component.cpu().numpy())
    for k in ("vertices", "triangles", "edges", "open_edges"):
        assert torch.equal(getattr(gpu, k), getattr(plain, k)), k
    # the same terms in another order: both sums carry at most (10 + n / 256) roundings of size 2^-53 relative to the sum of the
    # magnitudes, which is the area itself and, for the volume (|p| <= 1), at most a third of it
    n, area = plain.triangles.item(), plain.area.item()
    bound = 2 * (10 + n / 256) * 2.0 ** -53 * area
    assert abs(gpu.area.item() - area) <= bound and abs(gpu.volume.item() - plain.volume.item()) <= bound / 3
    kept = T.keep_components(shuffled, gpu, torch.ones(1))
    assert K.same_batches(kept, shuffled)


def ribbon_batch(count, triangles, seed):
    return K.pack([K.ribbon(triangles, seed + i) for i in range(count)], "cuda")


def test_long_ribbon_with_random_numbering():
    batch = ribbon_batch(1, 200000, 9)
    gpu, _ = check_against_twin(batch)
    n = 200000
    assert len(gpu) == 1 and (gpu.vertex_component == 0).all()
    assert (gpu.vertices.item(), gpu.triangles.item(), gpu.edges.item(), gpu.open_edges.item()) == (n + 2, n, 2 * n + 1, n + 2)
    assert np.array_equal(gpu.vertex_component.cpu().numpy(), reference_labels(batch))
    shuffled, perm = K.permuted(batch, 6)
    again = T.components(shuffled)
    assert R.same_partition(again.vertex_component.cpu().numpy()[perm.cpu().numpy()], gpu.vertex_component.cpu().numpy())
    assert K.same_batches(T.keep_components(batch, gpu, torch.ones(1)), batch)


def test_batch_of_ribbons():
    batch = ribbon_batch(64, 4000, 100)
    gpu, cpu = check_against_twin(batch, rules=("largest",))
    assert gpu.counts().tolist() == [1] * 64 and gpu.triangles.tolist() == [4000] * 64 and gpu.open_edges.tolist() == [4002] * 64
    assert np.array_equal(gpu.vertex_component.cpu().numpy(), reference_labels(batch))
    mask = torch.arange(64) % 3 != 1
    kept = T.keep_components(batch, gpu, mask.cuda())
    assert K.same_batches(kept, T.keep_components(to_cpu(batch), cpu, mask))
    assert kept.triangle_counts().tolist() == [4000 if m else 0 for m in mask.tolist()]


# ---- clean= on the device -------------------------------------------------------------------------------------------------------------
def reference_clean(batch, rule):
    """The reference's cleaning of a device batch, as a MeshBatch on that device."""
    ref = R.components(batch)
    v, n, f, vo, to = R.compact(batch, ref, R.select(ref, rule))
    dev = batch.vertices.device
    return MeshBatch(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (v, n, f, vo, to))), ref


def test_clean_through_get_mesh_and_sample_point_clouds():
    import project_forms
    from shapegan_amd.surface import cell_diagonal, refine_meshes
    net = project_forms.chairs_net("cuda")[0]
    codes = torch.stack([torch.randn(128, generator=torch.Generator().manual_seed(s)) for s in (2, 3)]).cuda()
    res, pieces = 32, []
    for z in codes:
        plain = net.get_mesh(z, res, sphere_only=False, narrow_band=True)
        batch = MeshBatch(torch.from_numpy(plain.vertices).cuda(), torch.from_numpy(plain.vertex_normals).cuda(),
                          torch.from_numpy(plain.faces).cuda(), torch.tensor([0, len(plain.vertices)]).cuda(),
                          torch.tensor([0, len(plain.faces)]).cuda())
        expected, ref = reference_clean(batch, "largest")
        pieces.append(len(ref["area"]))
        got = net.get_mesh(z, res, sphere_only=False, narrow_band=True, clean="largest")
        assert np.array_equal(got.vertices, expected.vertices.cpu().numpy()) and np.array_equal(got.faces, expected.faces.cpu().numpy())
        assert got.body_count == 1
        refined = refine_meshes(net, z.reshape(1, -1), expected, level=0, iterations=2, max_move=cell_diagonal(res))[0].mesh(0)
        got = net.get_mesh(z, res, sphere_only=False, narrow_band=True, refine=2, clean="largest")
        assert np.array_equal(got.vertices, refined.vertices) and np.array_equal(got.vertex_normals, refined.vertex_normals)
        assert np.array_equal(got.faces, refined.faces)
    assert max(pieces) > 1, "neither mesh had a floater to remove: %s" % pieces
    # sample_point_clouds: the clouds of the device's own meshes, cleaned by the reference
    with torch.no_grad():
        grids = net.voxel_grids(codes, res, sphere_only=False, level=metrics.LEVEL)
    batch = marching_cubes(grids, level=metrics.LEVEL, spacing=2 / res, origin=-1, pad=True, pad_value=1.0)
    for rule in ("largest", True):
        got = metrics.sample_point_clouds(net, 2, 300, voxel_resolution=res, latent_codes=codes, generator=torch.Generator().manual_seed(4),
                                          clean=rule)
        points, empty = reference_clean(batch, rule)[0].sample_surface(300, generator=torch.Generator().manual_seed(4), return_empty=True)
        want = np.zeros((2, 300, 3))
        metrics._collect(want, 0, points, empty, "half_unit_sphere")
        assert np.array_equal(got, want)
    off = metrics.sample_point_clouds(net, 2, 300, voxel_resolution=res, latent_codes=codes, generator=torch.Generator().manual_seed(4), clean=False)
    assert np.array_equal(off, metrics.sample_point_clouds(net, 2, 300, voxel_resolution=res, latent_codes=codes,
                                                           generator=torch.Generator().manual_seed(4)))
