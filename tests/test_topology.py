"""Mesh topology on the C++ twin (no GPU): components, statistics, keep rules and compaction against tests/topology_reference.py, the
trimesh-named properties of Mesh, and clean= through the public meshing paths."""
import math

import numpy as np
import pytest
import torch

import topology_cases as K
import topology_reference as R
from shapegan_amd import metrics, topology as T
from shapegan_amd.mesh import Mesh, marching_cubes
from shapegan_amd.reconstruct import reconstruct_meshes
from test_mesh import closed_and_oriented, sphere_grid, torus_grid

RULES = ("largest", True, {"largest": 2}, {"min_area_fraction": 0.2}, {"min_triangles": 5}, {"drop_cavities": True},
         {"largest": 3, "min_triangles": 4, "drop_cavities": True, "min_area_fraction": 0.001})


def one(comps, name, c=0):
    return getattr(comps, name)[c].item()


# ---- hand-built meshes ---------------------------------------------------------------------------------------------------------------
def test_hand_meshes_against_the_reference():
    order, batch = K.hand_batch()
    comps = T.components(batch)
    ref = R.components(batch)
    R.check_against(comps, ref)
    assert comps.counts().tolist() == [0, 2, 1, 0, 1, 1, 0, 1, 1, 2, 0]
    assert comps.shape_index.tolist() == [1, 1, 2, 4, 5, 7, 8, 9, 9]


def shape(name):
    batch = K.pack([K.hand_meshes()[name]])
    return batch, T.components(batch)


def test_two_tetrahedra():
    _, c = shape("two_tetrahedra")
    assert len(c) == 2 and c.vertex_component.tolist() == [0] * 4 + [1] * 4
    assert c.watertight.tolist() == [True, True] and c.euler.tolist() == [2, 2] and c.genus.tolist() == [0, 0]
    assert c.vertices.tolist() == [4, 4] and c.triangles.tolist() == [4, 4] and c.edges.tolist() == [6, 6]
    assert c.volume[0].item() == pytest.approx(1 / 6, rel=1e-15) and c.area[0].item() == pytest.approx(1.5 + math.sqrt(3) / 2, rel=1e-15)


def test_open_triangle_and_unreferenced_vertex():
    _, c = shape("open_triangle")
    assert len(c) == 1 and one(c, "open_edges") == 3 and one(c, "edges") == 3 and not one(c, "watertight") and one(c, "genus") == -1
    batch, c = shape("unreferenced_vertex")
    assert c.vertex_component.tolist() == [-1, 0, 0, 0, 0] and one(c, "vertices") == 4 and one(c, "watertight")
    kept = T.keep_components(batch, c, torch.ones(1))
    assert kept.vertices.shape[0] == 4 and torch.equal(kept.faces, torch.from_numpy(K.TET_F))
    for name in ("no_triangles", "nothing"):
        batch, c = shape(name)
        assert len(c) == 0 and (c.vertex_component == -1).all() and c.comp_offsets.tolist() == [0, 0]
        assert c.summary()["watertight"].tolist() == [False]
        assert T.keep_components(batch, c, torch.zeros(0)).vertices.shape == (0, 3)


def test_tetrahedra_sharing_one_vertex_are_one_component_of_euler_3():
    _, c = shape("shared_vertex")
    assert len(c) == 1 and one(c, "euler") == 3 and one(c, "open_edges") == 0
    assert (one(c, "vertices"), one(c, "edges"), one(c, "triangles")) == (7, 12, 8)
    assert one(c, "volume") == pytest.approx(1 / 3, rel=1e-15)


def test_one_flipped_triangle_opens_its_edges():
    _, c = shape("one_flipped")
    assert len(c) == 1 and one(c, "open_edges") == 3 and one(c, "edges") == 6 and not one(c, "watertight")


def test_out_of_range_triangles_are_skipped_everywhere():
    batch, c = shape("out_of_range")
    _, plain = shape("two_tetrahedra")
    assert len(c) == 1 and one(c, "triangles") == 4 and one(c, "watertight")
    assert one(c, "area") == one(plain, "area") and one(c, "volume") == one(plain, "volume")
    kept = T.keep_components(batch, c, torch.ones(1))
    assert torch.equal(kept.faces, torch.from_numpy(K.TET_F)) and torch.equal(kept.vertices, batch.vertices)


def test_degenerate_triangle_connects_its_distinct_vertices():
    _, c = shape("degenerate")
    assert len(c) == 2 and c.vertex_component.tolist() == [0] * 4 + [1, 1]
    assert (one(c, "vertices", 1), one(c, "edges", 1), one(c, "triangles", 1), one(c, "open_edges", 1)) == (2, 1, 1, 0)      # its two
    # proper sides run 0 -> 1 and 1 -> 0: by the definition that edge is closed
    assert one(c, "area", 1) == 0.0


def test_bad_arguments_are_refused():
    batch = K.pack([K.tet()])
    comps = T.components(batch)
    with pytest.raises(ValueError):
        T.keep_components(batch, comps, torch.ones(3))
    with pytest.raises(ValueError):
        T.select(comps, "smallest")
    with pytest.raises(ValueError):
        T.select(comps, {"min_volume": 1.0})
    from shapegan_amd import lib as L
    lib = L.load()
    assert lib.sg_topo_label_workspace_bytes(0, 4) == 0 and lib.sg_topo_label_workspace_bytes(1, 1 << 31) == 0
    assert lib.sg_topo_keep_workspace_bytes(1, 4, 1 << 31) == 0 and lib.sg_topo_stats_workspace_bytes(1 << 31, 0) == 0
    label, co, ws = torch.empty(4, dtype=torch.int32), torch.empty(2, dtype=torch.int64), torch.empty(64, dtype=torch.int32)
    try:
        for S, V, F in ((0, 4, 4), (1, -1, 4), (1, 4, 1 << 31)):
            rc = lib.sg_topo_label(L.ptr(batch.faces), L.ptr(batch.vert_offsets), L.ptr(batch.tri_offsets), S, V, F, L.ptr(label),
                                   L.ptr(co), L.ptr(ws), 256, None)
            assert rc == -1, (S, V, F)
    finally:
        L.reset_call_state()


# ---- marching-cubes meshes -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solids():
    """sphere, torus, two spheres, shell: one batch, its components, the reference."""
    batch = K.mesh_grids(np.stack([sphere_grid(32, 0.6), torus_grid(32, 0.5, 0.2), K.two_spheres_grid(32), K.shell_grid(32)]))
    return batch, T.components(batch), R.components(batch)


def test_solids_against_the_reference(solids):
    batch, comps, ref = solids
    R.check_against(comps, ref)
    assert comps.counts().tolist() == [1, 1, 2, 2] and comps.watertight.all()
    assert comps.summary()["watertight"].tolist() == [True] * 4


def test_sphere_is_one_watertight_component_of_genus_0_and_the_right_volume(solids):
    _, comps, _ = solids
    assert comps.genus[0].item() == 0 and comps.euler[0].item() == 2
    # the vertices lie on the sphere up to the interpolation error h^2 / (8 r) of the convex distance along an edge, the triangles
    # (edges at most h sqrt 3) cut caps of sagitta 3 h^2 / (8 r) at most: radial error below h^2 / (2 r), three times that in volume
    r, h = 0.6, 2 / 31
    exact = 4 * math.pi * r ** 3 / 3
    assert abs(comps.volume[0].item() - exact) <= exact * 3 * h * h / (2 * r * r)


def test_torus_has_genus_1(solids):
    _, comps, _ = solids
    assert comps.genus[1].item() == 1 and comps.euler[1].item() == 0


def test_two_spheres_and_the_cavity(solids):
    batch, comps, _ = solids
    assert comps.genus[2:].tolist() == [0, 0, 0, 0]
    assert (comps.volume[2:4] > 0).all()
    outer, inner = sorted(comps.volume[4:6].tolist(), reverse=True)
    void = 4 * math.pi * 0.4 ** 3 / 3
    assert outer > 0 > inner and abs(inner + void) <= void * 3 * (2 / 31) ** 2 / (2 * 0.4 ** 2)      # the sphere's bound, r = 0.4
    assert comps.summary()["volume"][3].item() == pytest.approx(outer + inner, rel=1e-15)
    cleaned, found = T.clean_meshes(batch, {"drop_cavities": True})
    assert found.kept.tolist() == [True, True, True, True] + [v > 0 for v in comps.volume[4:6].tolist()]
    after = T.components(cleaned)
    assert after.counts().tolist() == [1, 1, 2, 1] and (after.volume > 0).all()


@pytest.fixture(scope="module")
def noise():
    batch = K.mesh_grids(K.noise_grids(6, 16, 3))
    return batch, T.components(batch), R.components(batch)


def test_noise_grids_have_hundreds_of_components(noise):
    batch, comps, ref = noise
    assert len(comps) > 200 and int(comps.counts().min()) > 20
    R.check_against(comps, ref)
    assert comps.watertight.all()      # marching cubes closes every piece
    s = T.summary(batch)
    assert s["mean_components"] == pytest.approx(len(comps) / 6) and s["single_component_fraction"] == 0.0 and s["watertight_fraction"] == 1.0
    share = [ref["area"][a:b].max() / ref["area"][a:b].sum() for a, b in zip(ref["comp_offsets"][:-1], ref["comp_offsets"][1:])]
    assert s["mean_largest_area_fraction"] == pytest.approx(np.mean(share), rel=1e-12)


# ---- keep rules and compaction -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES, ids=[str(i) for i in range(len(RULES))])
@pytest.mark.parametrize("which", ["hand", "solids", "noise"])
def test_keep_rules_against_the_reference(which, rule, solids, noise):
    batch, comps, ref = {"solids": solids, "noise": noise}.get(which) or (lambda b: (b, T.components(b), R.components(b)))(K.hand_batch()[1])
    mask = T.select(comps, rule)
    expected = R.select(ref, rule)
    assert mask.tolist() == expected.tolist()
    kept = T.keep_components(batch, comps, mask)
    assert K.equals_reference(kept, R.compact(batch, ref, expected))
    cleaned, found = T.clean_meshes(batch, rule)
    assert K.same_batches(cleaned, kept) and K.same_batches(batch.clean(rule), kept) and found.kept.tolist() == expected.tolist()
    if which != "hand":
        for m in kept.meshes():
            assert closed_and_oriented(m.faces)
        again = T.components(kept)
        assert len(again) == int(expected.sum()) and again.watertight.all()
        assert torch.equal(again.area, comps.area[mask]) and torch.equal(again.triangles, comps.triangles[mask])


def test_keep_all_is_the_batch_and_keep_none_is_empty(noise, solids):
    for batch, comps, _ in (noise, solids):
        assert K.same_batches(T.keep_components(batch, comps, torch.ones(len(comps), dtype=torch.bool)), batch)
        none = T.keep_components(batch, comps, torch.zeros(len(comps), dtype=torch.bool))
        assert none.vertices.shape == (0, 3) and none.faces.shape == (0, 3) and none.normals.shape == (0, 3)
        assert none.vert_offsets.tolist() == [0] * (len(batch) + 1) and none.tri_offsets.tolist() == [0] * (len(batch) + 1)
        assert len(T.components(none)) == 0


def test_largest_breaks_ties_toward_the_lower_number():
    batch = K.pack([K.join(K.tet(), K.tet(3.0), K.tet(-3.0))])
    comps = T.components(batch)
    assert comps.area[0].item() == comps.area[0].item() and T.select(comps, "largest").tolist() == [True, False, False]
    assert T.select(comps, {"largest": 2}).tolist() == [True, True, False]


# ---- the trimesh names on Mesh -------------------------------------------------------------------------------------------------------
def test_mesh_properties(solids):
    batch, comps, _ = solids
    two = batch.mesh(2)
    assert two.body_count == 2 and two.is_watertight and two.euler_number == 4
    assert two.volume == pytest.approx(float(comps.volume[2:4].sum()), rel=1e-12)
    parts = two.split()
    assert [len(p.faces) for p in parts] == comps.triangles[2:4].tolist()
    assert sum(len(p.vertices) for p in parts) == len(two.vertices)
    for p, c in zip(parts, (2, 3)):
        assert p.body_count == 1 and p.is_watertight and closed_and_oriented(p.faces)
        assert p.volume == comps.volume[c].item() and p.vertex_normals.shape == p.vertices.shape
    assert batch.mesh(1).euler_number == 0 and batch.mesh(3).body_count == 2
    v, f = K.hand_meshes()["open_triangle"]
    m = Mesh(v, f)
    assert m.body_count == 1 and not m.is_watertight and m.volume == 0.0 and m.euler_number == 1 and m.split()[0].vertex_normals is None
    assert Mesh(v, f[:0]).body_count == 0 and not Mesh(v, f[:0]).is_watertight and Mesh(v, f[:0]).split() == []
    assert batch.components().counts().tolist() == comps.counts().tolist()


# ---- clean= through the public paths (chairs weights) --------------------------------------------------------------------------------
SEEDS = range(8)
RES = 32


@pytest.fixture(scope="module")
def chairs():
    """The trained chairs network on the twin, the codes of seeds 0..7 and their uncleaned meshes (one batch)."""
    import project_forms
    net = project_forms.chairs_net("cpu")[0]
    codes = torch.stack([torch.randn(128, generator=torch.Generator().manual_seed(s)) for s in SEEDS])
    with torch.no_grad():
        grids = net.voxel_grids(codes, RES, sphere_only=False, level=0)
    batch = marching_cubes(grids, level=0, spacing=2 / RES, origin=-1, pad=True, pad_value=1.0)
    return net, codes, batch, grids


def test_most_random_codes_give_more_than_one_component(chairs):
    batch = chairs[2]
    counts = T.components(batch).counts().tolist()
    print("[topology] components of seeds 0..7 at %d^3: %s" % (RES, counts))
    assert sum(c > 1 for c in counts) >= 6


@pytest.mark.parametrize("rule", ["largest", True, {"largest": 2, "min_triangles": 8}], ids=["largest", "default", "dict"])
def test_get_mesh_clean_equals_clean_meshes_of_the_uncleaned_mesh(chairs, rule):
    net, codes, batch, _ = chairs
    cleaned = T.clean_meshes(batch, rule)[0]
    shrunk = 0
    for s in (2, 3):
        plain = net.get_mesh(codes[s], RES, sphere_only=False)
        assert np.array_equal(plain.vertices, batch.mesh(s).vertices) and np.array_equal(plain.faces, batch.mesh(s).faces)
        for off in (net.get_mesh(codes[s], RES, sphere_only=False, clean=False),):
            assert np.array_equal(off.vertices, plain.vertices) and np.array_equal(off.faces, plain.faces)
            assert np.array_equal(off.vertex_normals, plain.vertex_normals)
        got, want = net.get_mesh(codes[s], RES, sphere_only=False, clean=rule), cleaned.mesh(s)
        assert np.array_equal(got.vertices, want.vertices) and np.array_equal(got.faces, want.faces)
        assert np.array_equal(got.vertex_normals, want.vertex_normals)
        assert len(got.faces) <= len(plain.faces) and closed_and_oriented(got.faces)
        shrunk += len(got.faces) < len(plain.faces)
        if rule == "largest":
            assert got.body_count == 1 and len(got.faces) < len(plain.faces)      # both seeds carry floaters
    assert shrunk > 0, "the rule removed nothing from either mesh"
    # nothing left counts as an empty mesh
    assert net.get_mesh(codes[0], RES, sphere_only=False, clean={"min_triangles": 10 ** 9}) is None
    with pytest.raises(ValueError):
        net.get_mesh(codes[0], RES, sphere_only=False, clean={"min_triangles": 10 ** 9}, raise_on_empty=True)


def test_sample_point_clouds_clean_samples_the_cleaned_batch(chairs):
    net, codes = chairs[0], chairs[1][:3]
    batch = marching_cubes(chairs[3][:3], level=0, spacing=2 / RES, origin=-1, pad=True, pad_value=1.0)
    n = 200

    def gen():
        return torch.Generator().manual_seed(11)
    for rule in ("largest",):
        got = metrics.sample_point_clouds(net, len(codes), n, voxel_resolution=RES, latent_codes=codes, generator=gen(), clean=rule)
        points, empty = T.clean_meshes(batch, rule)[0].sample_surface(n, generator=gen(), return_empty=True)
        want = np.zeros((len(codes), n, 3))
        metrics._collect(want, 0, points, empty, "half_unit_sphere")
        assert np.array_equal(got, want)
    plain = metrics.sample_point_clouds(net, len(codes), n, voxel_resolution=RES, latent_codes=codes, generator=gen())
    off = metrics.sample_point_clouds(net, len(codes), n, voxel_resolution=RES, latent_codes=codes, generator=gen(), clean=False)
    assert np.array_equal(plain, off) and not np.array_equal(plain, got)
    # voxel grids: the same through sample_from_voxels
    grids = K.noise_grids(2, 16, 5)
    torch.manual_seed(3)
    got = metrics.sample_from_voxels(grids, 50, clean="largest")
    torch.manual_seed(3)
    points, empty = marching_cubes(grids, level=0, spacing=2 / 16, origin=-1).clean("largest").sample_surface(50, return_empty=True)
    want = np.zeros((2, 50, 3))
    metrics._collect(want, 0, points, empty, "half_unit_sphere")
    assert np.array_equal(got, want)
    torch.manual_seed(3)
    a = metrics.sample_from_voxels(grids, 50)
    torch.manual_seed(3)
    assert np.array_equal(a, metrics.sample_from_voxels(grids, 50, clean=False))


def test_reconstruct_meshes_clean(chairs):
    net, codes = chairs[0], chairs[1]
    plain = reconstruct_meshes(net, codes[:2], RES)
    assert K.same_batches(reconstruct_meshes(net, codes[:2], RES, clean=False), plain)
    for rule in ("largest", True):
        assert K.same_batches(reconstruct_meshes(net, codes[:2], RES, clean=rule), T.clean_meshes(plain, rule)[0])
    # cleaning comes before refine: the refined vertices are those of the cleaned mesh
    from shapegan_amd.surface import cell_diagonal, refine_meshes
    want = refine_meshes(net, codes[:2], T.clean_meshes(plain, "largest")[0], iterations=2, max_move=cell_diagonal(RES))[0]
    assert K.same_batches(reconstruct_meshes(net, codes[:2], RES, clean="largest", refine=2), want)


def test_traversal_frames_clean(chairs):
    from shapegan_amd.traversal import clean_option, traversal_frames
    net, codes = chairs[0], chairs[1]

    from project_forms import _CaptureRenderer as Capture
    plain, off, cleaned = Capture(), Capture(), Capture()
    assert list(traversal_frames(net, codes[:3], voxel_resolution=16, level=0.0, renderer=plain)) == []
    assert list(traversal_frames(net, codes[:3], voxel_resolution=16, level=0.0, renderer=off, clean=False)) == []
    assert list(traversal_frames(net, codes[:3], voxel_resolution=16, level=0.0, renderer=cleaned, clean="largest")) == []
    assert K.same_batches(plain.batches[0], off.batches[0])
    assert K.same_batches(cleaned.batches[0], T.clean_meshes(plain.batches[0], "largest")[0])
    assert (clean_option(None), clean_option("default"), clean_option("largest")) == (False, True, "largest")
