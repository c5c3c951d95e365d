"""Bodies shared by tests/test_brickgrid.py and tests/test_gpu_brickgrid.py: the narrow-band path of SDFNet.voxel_grids and of its
callers with the chairs network, against the dense path.

Codes: the golden code z of tests/golden/sdfnet_examples.npz, z / 2 and -z.  band = 0.02: the network's values are clamped to about
+-0.1, so the default band (0.17 at 32^3 with bricks of 4) would make every brick active at these resolutions and nothing of the
continuation would run.
"""
import os

import numpy as np
import torch

import brickgrid_forms as F
import latent_fit_forms as LF
from shapegan_amd.mesh import marching_cubes

BAND = 0.02
CASES = [(R, B, so, level) for R in (16, 32) for B in (4, 8) for so in (True, False) for level in (0.0, 0.04)]

# (R, B, sphere_only, level, code) whose dense mesh has a piece that the narrow-band mesh lacks at BAND: the piece's lattice points
# lie in inactive bricks that no corner came within BAND of (at (16, 4, False, 0, 2) one of its crossing edges leaves such a brick: its
# other end is an evaluated point on the side of the brick's fill, which is why nothing follows it).  Found by running
# every case on the CPU twin and comparing the two meshes; at (16, 8) and level 0 the 2 x 2 x 2 bricks have no corner within BAND
# of the surface of code 0 and none inside it, so that whole shape counts as such a piece.
FLOATERS = {(16, 8, True, 0.0, 0), (16, 8, False, 0.0, 0), (16, 4, False, 0.0, 2), (32, 4, True, 0.0, 2), (32, 4, False, 0.0, 2),
            (32, 8, False, 0.0, 2)}

_cache = {}


def codes(dev):
    z = torch.from_numpy(np.load(os.path.join(LF.GOLDEN, "sdfnet_examples.npz"))["z"]).float()
    return torch.stack([z, 0.5 * z, -z]).to(dev)


def net(dev):
    if ("net", dev) not in _cache:
        _cache["net", dev] = LF.net_on(dev, 5, 128, LF.chairs_state())
    return _cache["net", dev]


def dense(dev, R, sphere_only):
    """the dense grids [3,R,R,R] (no padding), computed once per resolution and shared"""
    key = ("dense", dev, R, sphere_only)
    if key not in _cache:
        _cache[key] = net(dev).voxel_grids(codes(dev), R, sphere_only=sphere_only, pad=False)
    return _cache[key]


def check_case(dev, R, B, sphere_only, level):
    d = dense(dev, R, sphere_only)
    g, stats = net(dev).voxel_grids(codes(dev), R, sphere_only=sphere_only, pad=False, narrow_band=True, level=level, brick=B, band=BAND,
                                    return_stats=True)
    assert g.shape == d.shape and g.dtype == d.dtype and g.device == d.device
    if R == 16:
        again = net(dev).voxel_grids(codes(dev), R, sphere_only=sphere_only, pad=False, narrow_band=True, level=level, brick=B, band=BAND)
        assert torch.equal(g, again)
    nbx = R // B
    for s in range(3):
        active = stats["active_bricks"][s]
        assert stats["evaluated_points"][s] == 8 * nbx ** 3 + active * B ** 3
        # every value that differs from the dense grid is the one constant of its brick: active points equal the dense grid bit for bit
        differs = (g[s] != d[s]).reshape(nbx, B, nbx, B, nbx, B).permute(0, 2, 4, 1, 3, 5).reshape(nbx ** 3, -1)
        assert not differs[(stats["state"][s] != 0)].any()
        dm = marching_cubes(d[s], level=level, spacing=2.0 / R, origin=-1.0, pad=True)
        nm = marching_cubes(g[s], level=level, spacing=2.0 / R, origin=-1.0, pad=True)
        F.assert_closed(nm)
        if (R, B, sphere_only, level, s) in FLOATERS:
            F.missing_triangles_lie_in_inactive_bricks(nm.mesh(0), dm.mesh(0), stats["state"][s].cpu().numpy(), R, B, strict=False)
        else:
            F.assert_same_mesh(nm, dm)


class Recorded(object):
    """wraps net.voxel_grids for the length of a `with`: the stats of every call it serves"""

    def __init__(self, network):
        self.net, self.stats = network, []

    def __enter__(self):
        original = self.net.voxel_grids

        def voxel_grids(*args, **kwargs):
            grids, stats = original(*args, **dict(kwargs, return_stats=True))
            self.stats.append(stats)
            return grids
        self.net.voxel_grids = voxel_grids
        return self

    def __exit__(self, *exc):
        del self.net.voxel_grids

    def assert_fewer_points(self, calls):
        assert len(self.stats) == calls
        for st in self.stats:
            assert st["rounds"] >= 1 and all(n < st["dense_points"] for n in st["evaluated_points"]), st


OPTIONS = dict(brick=4, band=BAND)


def check_get_mesh(dev):
    n, z = net(dev), codes(dev)
    for level in (0.0, 0.04):
        want = n.get_mesh(z[0], 32, level=level)
        with Recorded(n) as rec:
            got = n.get_mesh(z[0], 32, level=level, narrow_band=OPTIONS)
        rec.assert_fewer_points(1)
        assert rec.stats[0]["level"] == level, "the brick grid is built for the level it is meshed at"
        for name in ("vertices", "faces", "vertex_normals"):
            assert np.array_equal(getattr(got, name), getattr(want, name))


def check_sample_point_clouds(dev):
    from shapegan_amd import metrics
    n, z = net(dev), codes(dev)[:2]
    gdev = "cuda" if dev == "cuda" else "cpu"
    want = metrics.sample_point_clouds(n, 2, 64, voxel_resolution=32, latent_codes=z, generator=torch.Generator(gdev).manual_seed(7))
    with Recorded(n) as rec:
        got = metrics.sample_point_clouds(n, 2, 64, voxel_resolution=32, latent_codes=z, narrow_band=OPTIONS,
                                          generator=torch.Generator(gdev).manual_seed(7))
    rec.assert_fewer_points(1)
    assert np.array_equal(got, want) and np.abs(want).sum() > 0


def check_traversal_frames(dev):
    from shapegan_amd import traversal as T
    n, z = net(dev), codes(dev)[:2]
    want = list(T.traversal_frames(n, z, voxel_resolution=32, size=32))
    with Recorded(n) as rec:
        got = list(T.traversal_frames(n, z, voxel_resolution=32, size=32, narrow_band=OPTIONS))
    rec.assert_fewer_points(1)
    assert rec.stats[0]["level"] == T.SURFACE_LEVEL
    assert len(got) == len(want) == 2 and all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    assert not np.array_equal(got[0], got[1])


def check_reconstruct_meshes(dev):
    from shapegan_amd import reconstruct
    n, z = net(dev), codes(dev)[:2]
    want = reconstruct.reconstruct_meshes(n, z, 32, level=0.04)
    with Recorded(n) as rec:
        got = reconstruct.reconstruct_meshes(n, z, 32, level=0.04, narrow_band=OPTIONS)
    rec.assert_fewer_points(1)
    F.assert_same_mesh(got, want)


def check_position_independence(dev):
    """One launch of 3 x 512 points through sg_sdfnet_fwd in dense order (points_period: shape s takes points 512 s ...) and in
    shuffled brick order with a shape index per point gives equal bits: what the guarantee of K18 rests on."""
    from shapegan_amd import ops
    n, z = net(dev), codes(dev)
    pts = (torch.rand(512, 3, generator=torch.Generator().manual_seed(11)) * 2 - 1).to(dev)
    want = n.grid_values(z, pts)                                        # [3, 512], points_period = 512
    perm = torch.randperm(3 * 512, generator=torch.Generator().manual_seed(12)).to(dev)
    sid = (perm // 512).to(torch.int32).contiguous()
    shuffled = pts[perm % 512].contiguous()
    lib = ops._lib()
    packed, zb1, zb5 = n._pack_shapes.get_with_fold(n._params(), ops.f32c(z))
    out = torch.empty(3 * 512, dtype=torch.float32, device=pts.device)
    ops.check(lib.sg_sdfnet_fwd(ops.ptr(shuffled), 0, None, None, z.shape[1], ops.ptr(packed), 3, ops.ptr(zb1), ops.ptr(zb5), 3 * 512,
                                ops.ptr(sid), ops.ptr(out), None, 3 * 512, 3 * 512, ops.stream()), "sdfnet_fwd")
    assert torch.equal(out, want.reshape(-1)[perm])
