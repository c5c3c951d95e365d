"""Marching cubes and surface sampling on the MI355X (csrc/mesh.hip) against the C++ twin; SDFNet.get_mesh and metrics on the GPU."""
import numpy as np
import pytest
import torch

from shapegan_amd import metrics
from shapegan_amd.mesh import marching_cubes, sample_packed
from shapegan_amd.model.sdf_net import SDFNet
import geometry_reference as R
import test_mesh_reference as T
from test_mesh import closed_and_oriented, sphere_grid, torus_grid

pytestmark = pytest.mark.gpu


def mixed_batch(S, R, seed):
    """Seeded mix of sphere / torus SDF grids and uniform-noise grids."""
    g = torch.Generator().manual_seed(seed)
    out = torch.empty((S, R, R, R))
    for s in range(S):
        kind = s % 3
        if kind == 0:
            out[s] = torch.from_numpy(sphere_grid(R, 0.3 + 0.5 * float(torch.rand(1, generator=g))))
        elif kind == 1:
            out[s] = torch.from_numpy(torus_grid(R, 0.5, 0.1 + 0.2 * float(torch.rand(1, generator=g))))
        else:
            out[s] = torch.rand((R, R, R), generator=g) * 2 - 1
    return out


def assert_same_meshes(gpu, cpu):
    assert torch.equal(gpu.vert_offsets.cpu(), cpu.vert_offsets)
    assert torch.equal(gpu.tri_offsets.cpu(), cpu.tri_offsets)
    assert torch.equal(gpu.faces.cpu(), cpu.faces)
    torch.testing.assert_close(gpu.vertices.cpu(), cpu.vertices, rtol=0, atol=1e-6)
    torch.testing.assert_close(gpu.normals.cpu(), cpu.normals, rtol=0, atol=1e-6)


@pytest.mark.parametrize("name", ["sphere", "torus", "noise0", "noise1", "noise2"])
def test_gpu_matches_twin_single(name):
    if name == "sphere":
        g = torch.from_numpy(sphere_grid(32, 0.6))
    elif name == "torus":
        g = torch.from_numpy(torus_grid(32))
    else:
        g = torch.rand((16, 16, 16), generator=torch.Generator().manual_seed(int(name[-1]))) * 2 - 1
    for pad in (True, False):
        kw = dict(level=0.0, spacing=(2 / 31, 0.07, 0.05), origin=(-1, -0.5, 0.25), pad=pad)
        gpu, cpu = marching_cubes(g.cuda(), **kw), marching_cubes(g, **kw)
        assert_same_meshes(gpu, cpu)
        assert closed_and_oriented(gpu.faces.cpu().numpy()) or not pad


def test_gpu_matches_twin_batch_and_is_deterministic():
    grids = mixed_batch(100, 32, 7)
    kw = dict(level=0.0, spacing=2 / 32, origin=-1)
    gpu = marching_cubes(grids.cuda(), **kw)
    assert_same_meshes(gpu, marching_cubes(grids, **kw))
    again = marching_cubes(grids.cuda(), **kw)
    for a, b in ((gpu.vertices, again.vertices), (gpu.normals, again.normals), (gpu.faces, again.faces),
                 (gpu.vert_offsets, again.vert_offsets), (gpu.tri_offsets, again.tri_offsets)):
        assert torch.equal(a, b)


def test_gpu_sampling_matches_twin():
    grids = torch.stack([torch.from_numpy(sphere_grid(32, r)) for r in (0.3, 0.5, 0.7, 0.9)] + [torch.ones(32, 32, 32)])
    kw = dict(spacing=2 / 31, origin=-1 - 2 / 31)
    gpu, cpu = marching_cubes(grids.cuda(), **kw), marching_cubes(grids, **kw)
    u = torch.rand((5, 20000, 3), generator=torch.Generator().manual_seed(11))
    pg, eg = sample_packed(gpu.vertices, gpu.faces, gpu.vert_offsets, gpu.tri_offsets, u.cuda())
    pc, ec = sample_packed(cpu.vertices, cpu.faces, cpu.vert_offsets, cpu.tri_offsets, u)
    assert eg.tolist() == ec.tolist() == [0, 0, 0, 0, 1]
    pg = pg.cpu()
    assert (pg[4] == 0).all()
    # the GPU adds the cumulative areas as a tree, the twin in sequence (both in double): a sample whose u0 * total falls within
    # rounding of a boundary between two triangles may pick the neighbour — a tiny fraction, still on the surface
    diff = (pg - pc).abs().amax(dim=2)
    assert float((diff > 1e-5).float().mean()) < 1e-3
    for s, r in enumerate((0.3, 0.5, 0.7, 0.9)):
        assert float((pg[s].norm(dim=1) - r).abs().max()) < 0.02


@pytest.mark.parametrize("shape", R.MC_SHAPES)
def test_gpu_marching_cubes_against_reference(shape):
    """csrc/mesh.hip against the direct numpy reference (vertex order, faces and offsets exact; positions and normals in float64)
    and, on the same non-cubic shapes, levels and pad values, against the twin."""
    _, done = T.body_mc("cuda", shape)
    for grids, kw, gpu in done:
        assert_same_meshes(gpu, marching_cubes(grids, spacing=R.MC_SPACING, origin=R.MC_ORIGIN, **kw))


def test_gpu_marching_cubes_many_blocks():
    _, done = T.body_mc("cuda", (33, 32, 31), S=7, combos={(True, 0)})
    for grids, kw, gpu in done:
        assert_same_meshes(gpu, marching_cubes(grids, spacing=R.MC_SPACING, origin=R.MC_ORIGIN, **kw))


def test_gpu_surface_sampling_against_reference():
    T.body_sampling("cuda")


def test_gpu_sample_surface_reproducible():
    batch = marching_cubes(mixed_batch(6, 24, 3).cuda(), spacing=1 / 12, origin=-1)
    a = batch.sample_surface(4096, generator=torch.Generator(device="cuda").manual_seed(1))
    b = batch.sample_surface(4096, generator=torch.Generator(device="cuda").manual_seed(1))
    assert a.is_cuda and a.shape == (6, 4096, 3) and torch.equal(a, b)


def chairs_net(chairs_state):
    net = SDFNet()
    net.load_state_dict(chairs_state)
    net.eval()
    return net


@pytest.mark.parametrize("sphere_only", [True, False])
def test_get_mesh_chairs(chairs_state, sphere_only):
    net = chairs_net(chairs_state)
    z = (torch.randn(128, generator=torch.Generator().manual_seed(21)) * 0.5).cuda()
    for R in (32, 64):
        grid = net.voxel_grids(z[None], R, sphere_only=sphere_only)[0].cpu().numpy()
        assert np.array_equal(grid, net.get_voxels(z, R, sphere_only=sphere_only))
        m = net.get_mesh(z, voxel_resolution=R, sphere_only=sphere_only)
        assert m is not None and len(m.faces) > 500
        assert closed_and_oriented(m.faces)
    # vertex normals against the SDF's own gradient at the vertices, mapped back to the SDF's coordinates: sample index
    # i = (v + 1) R / 2 - pads sits at -1 + i 2 / (R - 1).  The grid normal is a central difference over two voxels, and the
    # learned chair field bends below that scale (thin legs and slats): measured on the twin, the mean angle is 16.6 deg at 32^3,
    # 11.3 at 64^3 and 7.2 at 128^3 (median 10.4 / 5.7 / 3.6), while the analytic sphere of tests/test_mesh.py is within 0.5 deg.
    # Checked at 64^3: the directions agree (median) and point the same way almost everywhere.
    pads = 1 if sphere_only else 2
    idx = (m.vertices.astype(np.float64) + 1) * R / 2 - pads
    pts = torch.from_numpy((-1 + idx * 2 / (R - 1)).astype(np.float32)).cuda()
    n = net.get_normals(z, pts).detach().cpu().numpy()
    cos = np.clip(np.einsum("ij,ij->i", n, m.vertex_normals), -1, 1)
    angle = np.degrees(np.arccos(cos))
    assert np.median(angle) < 7 and angle.mean() < 13
    assert (cos > 0).mean() > 0.97


def test_sample_point_clouds_gpu(chairs_state):
    net = chairs_net(chairs_state)
    z = (torch.randn(16, 128, generator=torch.Generator().manual_seed(22)) * 0.5).cuda()
    out = metrics.sample_point_clouds(net, 16, 2048, voxel_resolution=32, latent_codes=z)
    assert out.shape == (16, 2048, 3) and out.dtype == np.float64
    assert np.isclose(np.linalg.norm(out, axis=2).max(axis=1), 0.5).all()
    grids = net.voxel_grids(z, 32, sphere_only=False).cpu().numpy()
    for s in (0, 7, 15):
        assert np.array_equal(grids[s], net.get_voxels(z[s], 32, sphere_only=False))
