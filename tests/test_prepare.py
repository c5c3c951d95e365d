"""Meshes to SDF training data (shapegan_amd/prepare.py, K16) on the C++ twin against the float64 statement in prepare_reference.py.

The bodies take the device, so that test_gpu_prepare.py runs the same checks on the MI355X.  Bounds (prepare_reference): distances
within 16 * 2^-24 absolute of the float64 minimum; the sign exact for every point further than 2 texels from the surface.
Largest errors seen (twin and MI355X alike, the results are bit-identical): see DESIGN 3.12.
"""
import os

import numpy as np
import pytest
import torch

from shapegan_amd import datasets
from shapegan_amd import prepare as P
from shapegan_amd.rendering import raster
import prepare_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_soup(parts, dev):
    """A raster.Soup of the triangle arrays `parts` ([T_s, 3, 3] float32 each, possibly empty)."""
    counts = [len(p) for p in parts]
    positions = np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1, 3, 3) for p in parts])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return raster.Soup(torch.from_numpy(positions).to(dev), None, torch.from_numpy(offsets).to(dev))


def run_distance(parts, points, dev, want_tri=True, want_closest=True, split=0):
    """numpy (dist2, tri, closest, split used) of sg_meshsdf_distance on points [S, Q, 3]."""
    out = P.mesh_distance(make_soup(parts, dev), torch.from_numpy(np.array(points, dtype=np.float32)).to(dev), want_tri,
                          want_closest, split)
    return tuple(None if t is None else t.cpu().numpy() for t in out[:3]) + (out[3],)


def assert_same_bits(got, want, what=""):
    for g, w in zip(got, want):
        assert (g is None) == (w is None), what
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, what
            np.testing.assert_array_equal(g.view(np.uint8), w.view(np.uint8), err_msg=what)


# ---- distance against float64 -----------------------------------------------------------------------------------------------------------
def check_distance(name, dev):
    tris, queries, ref = R.distance_case(name)
    T = len(tris)
    dist2, tri, closest, _ = run_distance([tris], queries[None], dev)
    dist2, tri, closest = dist2[0], tri[0], closest[0]
    assert dist2.dtype == np.float32 and tri.dtype == np.int32 and closest.dtype == np.float32
    assert not np.isnan(dist2).any() and not np.isnan(closest).any()
    want = ref.min(axis=1)
    err = np.abs(np.sqrt(dist2).astype(np.float64) - want)
    print("%s on %s: largest distance error %.3g x 2^-24 (bound 16)" % (name, dev, err.max() / R.U))
    assert (err <= R.DIST_ATOL).all()
    assert (tri >= 0).all() and (tri < T).all()
    # neighbouring triangles tie only approximately: the index is checked through the float64 distance to the triangle it names
    of_tri = ref[np.arange(len(queries)), tri]
    assert (np.abs(of_tri - want) <= R.DIST_ATOL).all()
    # closest: at that distance from the query, and a point of the triangle `tri`
    q64 = queries.astype(np.float64)
    assert (np.abs(np.linalg.norm(q64 - closest, axis=1) - want) <= R.DIST_ATOL).all()
    on_tri = np.array([R.closest_points(closest[i:i + 1], tris[tri[i]:tri[i] + 1])[0][0, 0] for i in range(0, len(queries), 7)])
    assert (on_tri <= R.DIST_ATOL).all()
    # the 50 mesh vertices: exactly 0
    assert (dist2[-50:] == 0).all()


@pytest.mark.parametrize("name", sorted(R.MESHES))
def test_distance_matches_float64(name):
    check_distance(name, "cpu")


# ---- forms: the device against the twin bit for bit, and against float64 -----------------------------------------------------------------
def form_case(Q, T, seed=3):
    rng = np.random.RandomState(seed + Q * 31 + T)
    return R.random_soup(T, seed + T), rng.uniform(-1, 1, (1, Q, 3)).astype(np.float32)


def check_form(dev, Q, T, split=0):
    tris, points = form_case(Q, T)
    got = run_distance([tris], points, dev, split=split)
    assert_same_bits(got[:3], run_distance([tris], points, "cpu")[:3], "Q = %d, T = %d" % (Q, T))
    ref = R.closest_points(points[0], tris)[0].min(axis=1)
    assert (np.abs(np.sqrt(got[0][0]).astype(np.float64) - ref) <= R.DIST_ATOL).all()
    return got[3]


FORM_Q = (1, 63, 65, 257, 1000)
FORM_T = (1, P.CHUNK - 1, P.CHUNK, P.CHUNK + 1, 3 * P.CHUNK + 7)


@pytest.mark.parametrize("Q", FORM_Q)
def test_forms_query_counts(Q):
    check_form("cpu", Q, 300)


@pytest.mark.parametrize("T", FORM_T)
def test_forms_triangle_counts(T):
    check_form("cpu", 200, T)


def check_empty_middle_shape(dev):
    a, b = R.random_soup(40, 1), R.random_soup(300, 2)
    points = np.random.RandomState(5).uniform(-1, 1, (3, 130, 3)).astype(np.float32)
    parts = [a, np.zeros((0, 3, 3), np.float32), b]
    dist2, tri, closest, _ = got = run_distance(parts, points, dev)
    assert_same_bits(got[:3], run_distance(parts, points, "cpu")[:3])
    assert np.isposinf(dist2[1]).all() and (tri[1] == -1).all() and (closest[1] == 0).all()
    for s, part in ((0, a), (2, b)):
        alone = run_distance([part], points[s:s + 1], dev)
        assert_same_bits((dist2[s:s + 1], tri[s:s + 1], closest[s:s + 1]), alone[:3], "shape %d" % s)
        assert (tri[s] >= 0).all() and (tri[s] < len(part)).all()


def test_empty_middle_shape():
    check_empty_middle_shape("cpu")


def check_optional_outputs(dev):
    tris, points = form_case(65, 300)
    full = run_distance([tris], points, dev)
    for want_tri, want_closest in ((False, True), (True, False), (False, False)):
        got = run_distance([tris], points, dev, want_tri, want_closest)
        assert (got[1] is None) == (not want_tri) and (got[2] is None) == (not want_closest)
        np.testing.assert_array_equal(got[0], full[0])
        if want_tri:
            np.testing.assert_array_equal(got[1], full[1])
        if want_closest:
            np.testing.assert_array_equal(got[2].view(np.uint32), full[2].view(np.uint32))
    # the sign: sdf iff dist2, outside optional; one of them must be asked for
    depth, vps = rule_scan(dev)
    p = torch.from_numpy(points).to(dev)
    d2 = torch.from_numpy(full[0]).to(dev)
    sdf, outside = P.mesh_sign(p, depth, vps, 0.25, dist2=d2)
    sdf_only, none = P.mesh_sign(p, depth, vps, 0.25, dist2=d2, want_outside=False)
    none2, outside_only = P.mesh_sign(p, depth, vps, 0.25)
    assert none is None and none2 is None and torch.equal(sdf, sdf_only) and torch.equal(outside, outside_only)
    root = np.sqrt(full[0])      # numpy's float32 square root is the correctly rounded one
    np.testing.assert_array_equal(sdf.cpu().numpy(), np.where(outside.cpu().numpy() != 0, root, -root))
    with pytest.raises(RuntimeError, match="meshsdf_sign"):
        P.mesh_sign(p, depth, vps, 0.25, want_outside=False)


def test_optional_outputs():
    check_optional_outputs("cpu")


def check_on_the_triangle(dev):
    tris = R.random_soup(300, 9)
    t = tris[17].astype(np.float64)
    points = np.stack([t[0], t[1], t[2], (t[0] + t[1]) / 2, (t[1] + t[2]) / 2, t.mean(axis=0)]).astype(np.float32)[None]
    got = run_distance([tris], points, dev)
    assert_same_bits(got[:3], run_distance([tris], points, "cpu")[:3])
    assert (got[0][0, :3] == 0).all(), "a point on a corner is at distance exactly 0"
    assert (np.sqrt(got[0][0, 3:]) <= R.DIST_ATOL).all()


def test_points_on_the_triangle():
    check_on_the_triangle("cpu")


def check_non_finite(dev):
    """Non-finite points and corners: no fault, indices in [-1, T_s); the finite points far from the spoilt triangles keep their value."""
    tris = R.random_soup(300, 4)
    points = np.random.RandomState(6).uniform(-1, 1, (1, 70, 3)).astype(np.float32)
    bad_points = points.copy()
    bad_points[0, 3, 0], bad_points[0, 10, 1], bad_points[0, 20] = np.nan, np.inf, -np.inf
    dist2, tri, closest, _ = run_distance([tris], bad_points, dev)
    assert (tri >= -1).all() and (tri < 300).all()
    keep = np.ones(70, bool)
    keep[[3, 10, 20]] = False
    clean = run_distance([tris], points, dev)
    np.testing.assert_array_equal(dist2[0, keep], clean[0][0, keep])
    bad_tris = tris.copy()
    bad_tris[5, 1, 2], bad_tris[100, 0], bad_tris[299, 2, 0] = np.nan, np.inf, -np.inf
    dist2, tri, closest, _ = run_distance([bad_tris], points, dev)
    assert (tri >= -1).all() and (tri < 300).all()
    everything = bad_tris.copy()
    everything[:] = np.nan
    dist2, tri, closest, _ = run_distance([everything], points, dev)
    assert (tri >= -1).all() and (tri < 300).all()


def test_non_finite_inputs_stay_in_range():
    check_non_finite("cpu")


def check_sizes_refused(dev):
    """Sizes beyond the limits come back as SG_ERR_ARG (-1) from the entry points themselves, before any pointer is used."""
    lib = P.L.load()
    few = torch.zeros(64, dtype=torch.float32, device=dev)
    offsets = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)
    ptr, stream = P.L.ptr, P.L.stream
    for S, T, Q in ((65536, 1, 1), (0, 1, 1), (1, (1 << 24) + 1, 1), (1, 1, (1 << 24) + 1), (1, 1, 0), (32, 1, (1 << 24)), (1, -1, 1)):
        try:
            rc = lib.sg_meshsdf_distance(ptr(few), ptr(offsets), S, T, ptr(few), Q, ptr(few), None, None, ptr(ws), ws.numel(), stream())
        finally:
            P.L.reset_call_state()
        assert rc == -1, (S, T, Q)
        if T == 1:
            try:
                rc = lib.sg_meshsdf_sign(ptr(few), S, Q, ptr(few), raster._doubles(np.eye(4)), 1, 1, 0.5, None, None, ptr(ws), stream())
            finally:
                P.L.reset_call_state()
            assert rc == -1, (S, Q)
    for K, N, bias in ((0, 1, 0.5), (65, 1, 0.5), (1, 0, 0.5), (1, 16385, 0.5), (1, 1, -0.5), (1, 1, float("nan")), (1, 1, float("inf"))):
        try:
            rc = lib.sg_meshsdf_sign(ptr(few), 1, 1, ptr(few), raster._doubles(np.tile(np.eye(4), (65, 1, 1))), K, N, bias, None, None, ptr(ws), stream())
        finally:
            P.L.reset_call_state()
        assert rc == -1, (K, N, bias)
    with pytest.raises(ValueError, match="out of range"):
        run_distance([np.zeros((0, 3, 3), np.float32)] * 65536, np.zeros((65536, 1, 3), np.float32), dev)
    assert lib.sg_meshsdf_distance_workspace_bytes(1, 1 << 25, 1) == 0


def test_sizes_out_of_range_are_refused():
    check_sizes_refused("cpu")


# ---- the sign ------------------------------------------------------------------------------------------------------------------------------
SCANS = {}


def mesh_scans(dev, K, N):
    """The three meshes as one batch of scans at rho = 1, default bias; made once per (device, K, N)."""
    key = (dev, K, N)
    if key not in SCANS:
        SCANS[key] = P.SurfaceScans([R.mesh(n) for n in sorted(R.MESHES)], 1.0, K, N, device=dev)
    return SCANS[key]


def check_sign(dev, K, N, max_excluded):
    scans = mesh_scans(dev, K, N)
    names = sorted(R.MESHES)
    cases = [R.sign_case(n) for n in names]
    outside = scans.is_outside(np.stack([c[0] for c in cases])).cpu().numpy()
    margin = 2 * 2.0 * 1.0 / N      # 2 texels: 2 * (2 rho / N)
    for s, (name, (_, dist, inside)) in enumerate(zip(names, cases)):
        far = dist > margin
        wrong = int((outside[s][far] == inside[far]).sum())
        excluded = 1.0 - far.mean()
        print("%s on %s, K = %d, N = %d: %d wrong beyond 2 texels, %.1f %% of the points within the margin, %d wrong inside it"
              % (name, dev, K, N, wrong, 100 * excluded, int((outside[s][~far] == inside[~far]).sum())))
        assert excluded <= max_excluded, name
        assert wrong == 0, name


def test_sign_k20_n128():
    check_sign("cpu", 20, 128, 0.15)


def test_sign_k50_n256():
    check_sign("cpu", 50, 256, 0.10)


def rule_scan(dev):
    depth = np.array([[0.25, 1.0, -0.5, 0.0], [0.5, 0.125, 1.0, -0.25], [1.0, 0.75, 0.3, 0.9], [-0.9, 1.0, 0.6, 0.1]], dtype=np.float32)
    return torch.from_numpy(depth).to(dev).reshape(1, 1, 4, 4), np.eye(4, dtype=np.float64)[None]


def check_sign_rule(dev):
    """The written rule on a hand-made 4 x 4 map: in and out of the window, a cleared texel, in front of and behind t - bias by one ulp."""
    depth, vps = rule_scan(dev)
    bias = np.float32(0.5)
    d = depth.cpu().numpy()[0, 0]
    pts = []
    for iy in range(4):
        for ix in range(4):
            x, y = np.float32((ix + 0.5) / 2 - 1), np.float32(1 - (iy + 0.5) / 2)
            thr = np.float32(d[iy, ix] - bias)
            for z in (np.nextafter(thr, np.float32(-np.inf)), thr, np.nextafter(thr, np.float32(np.inf)), np.float32(-2), np.float32(2)):
                pts.append((x, y, z))
    for x, y in ((-1.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (np.nextafter(np.float32(1), np.float32(0)), 0.3), (-1.5, 0.2), (0.2, 1.5),
                 (0.3, -1.0000001), (np.nan, 0.0), (0.0, np.inf), (-np.inf, np.nan)):
        for z in (-2.0, 0.0, 2.0, np.nan):
            pts.append((x, y, z))
    pts.append((0.1, 0.1, np.nan))
    pts = np.asarray(pts, dtype=np.float32)
    _, outside = P.mesh_sign(torch.from_numpy(pts).to(dev)[None], depth, vps, float(bias))
    want = R.visible_rule(pts, d, vps[0], bias)
    np.testing.assert_array_equal(outside.cpu().numpy()[0].astype(bool), want)
    assert want.any() and not want.all()
    # two scans: the OR, and a point only the second one sees
    second = torch.ones_like(depth)
    _, both = P.mesh_sign(torch.from_numpy(pts).to(dev)[None], torch.cat([depth, second]), np.concatenate([vps, vps]), float(bias))
    assert both.bool().all()


def test_sign_rule_on_a_hand_made_map():
    check_sign_rule("cpu")


def check_perspective_is_refused(dev):
    depth, vps = rule_scan(dev)
    p = torch.zeros((1, 4, 3), device=dev)
    for row in ((0, 0, -1, 0), (0, 0, 0, 2), (1e-9, 0, 0, 1)):
        vp = vps.copy()
        vp[0, 3] = row
        with pytest.raises(RuntimeError, match="meshsdf_sign"):
            P.mesh_sign(p, depth, vp, 0.5)


def test_perspective_view_is_refused():
    check_perspective_is_refused("cpu")


# ---- the pipeline, K = 12, N = 64 --------------------------------------------------------------------------------------------------------
PIPE_K, PIPE_N = 12, 64
SNAP = 2 * (2 ** 0.5 / 512) * (2.0 / PIPE_N) + 4 * R.U      # at rho = 1: twice the largest move of a snapped corner, plus rounding


def check_voxels(dev):
    names = ["icosphere", "torus", "box"]
    scans = P.SurfaceScans([R.mesh(n) for n in names], 3 ** 0.5, PIPE_K, PIPE_N, device=dev)
    for res in (8, 16):
        voxels, ok = scans.get_voxels(res, check_result=True)
        assert voxels.shape == (3, res, res, res) and voxels.dtype == torch.float32 and ok.tolist() == [True, True, True]
        v = voxels.cpu().numpy()
        c = np.linspace(-1, 1, res)
        grid = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
        for s, n in enumerate(names):
            ref = R.closest_points(grid, R.soup(n))[0].min(axis=1).reshape(res, res, res)
            assert (np.abs(np.abs(v[s]) - ref) <= R.DIST_ATOL).all(), n      # grid points lie in [-1, 1]^3, the domain of the bound
            assert (v[s] < 0).any() and (v[s] > 0).any()
        # the axis order, on the box: half extents 0.5, 0.3, 0.4 hold 8, 4 and 6 of the 16 grid planes of axes 0, 1, 2
        inside = v[2] < 0
        extent = [int(inside.any(axis=tuple(a for a in range(3) if a != axis)).sum()) for axis in range(3)]
        assert res != 16 or extent == [8, 4, 6], extent
        # one flipped voxel makes a jump
        flipped = voxels.clone()
        flipped[0, 0, 0, 0] = -flipped[0, 0, 0, 0]
        assert P.check_voxels(flipped).tolist() == [False, True, True]
        assert P.check_voxels(voxels[1]) is True and P.check_voxels(flipped[0]) is False
    # the single form returns the same grid without the shape axis
    one = P.SurfaceScans(R.mesh("torus"), 3 ** 0.5, PIPE_K, PIPE_N, device=dev).get_voxels(8, check_result=True)
    assert torch.equal(one, scans.get_voxels(8)[1])


def test_voxels_pass_check_and_axes_are_in_order():
    check_voxels("cpu")


def check_near_surface(dev):
    scans = P.SurfaceScans(R.mesh("torus"), 1.0, PIPE_K, PIPE_N, device=dev)
    points, sdf = scans.sample_sdf_near_surface(2000, generator=torch.Generator().manual_seed(5))
    again = scans.sample_sdf_near_surface(2000, generator=torch.Generator().manual_seed(5))
    assert torch.equal(points, again[0]) and torch.equal(sdf, again[1])
    assert points.shape == (2000, 3) and sdf.shape == (2000,) and points.dtype == sdf.dtype == torch.float32
    ns = int(2000 * 47 / 50) // 2
    assert ns == 940
    p = points.cpu().numpy().astype(np.float64)
    dist = R.closest_points(p, R.soup("torus"))[0].min(axis=1)
    # a scan point lies on its triangle as the rasteriser snapped it: corners move by at most 1/512 texel per axis (8 sub-pixel bits),
    # so the point is within SNAP of the true surface; the noisy points lie within 5 sigma of it
    assert (dist[:ns] <= 5 * 0.0025 + SNAP).all() and (dist[ns:2 * ns] <= 5 * 0.00025 + SNAP).all()
    assert dist[:ns].mean() > 4 * dist[ns:2 * ns].mean()
    uniform = p[2 * ns:]
    assert len(uniform) == 120 and (np.linalg.norm(uniform, axis=1) < 1).all() and dist[2 * ns:].mean() > 0.1
    assert (np.abs(np.abs(sdf.cpu().numpy()) - dist) <= R.DIST_ATOL).all()
    # the two noisy groups share their surface points
    assert np.abs(p[:ns] - p[ns:2 * ns]).max() < 6 * 0.0025
    covered = scans.scan_points()
    assert covered.shape[1] == 3 and covered.shape[0] > 1000
    on_surface = R.closest_points(covered.cpu().numpy()[::37], R.soup("torus"))[0].min(axis=1)
    assert on_surface.max() <= SNAP


def test_near_surface_sampling():
    check_near_surface("cpu")


def check_uniform_and_surface(dev):
    scans = P.SurfaceScans([R.mesh("box"), R.single_triangle()], 1.0, PIPE_K, PIPE_N, device=dev)
    uniform, usdf, surface, ssdf, ok = scans.get_uniform_and_surface_points(3000, generator=torch.Generator().manual_seed(2))
    # nothing is inside a single triangle; what the bias calls inside lies within 2 rho / N of it on either side: at most
    # area * 2 * bias / (4 pi / 3) = 0.3 % of the unit sphere for this one, below the 1 % (and 1.5 %) that make a mesh bad
    assert ok.tolist() == [True, False]
    assert uniform.shape == surface.shape == (2, 3000, 3) and usdf.shape == ssdf.shape == (2, 3000)
    assert (uniform.norm(dim=2) < 1).all()
    u = uniform[0].cpu().numpy().astype(np.float64)
    ref = R.closest_points(u, R.soup("box"))[0].min(axis=1)
    assert (np.abs(np.abs(usdf[0].cpu().numpy()) - ref) <= R.DIST_ATOL).all()
    volume = 8 * 0.5 * 0.3 * 0.4 / (4 / 3 * np.pi)
    assert abs(float((usdf[0] < 0).float().mean()) - volume) < 0.03
    near = R.closest_points(surface[0].cpu().numpy(), R.soup("box"))[0].min(axis=1)
    assert (near <= 5 * 0.0025).all() and (np.abs(np.abs(ssdf[0].cpu().numpy()) - near) <= R.DIST_ATOL).all()
    with pytest.raises(P.BadMeshException):
        P.SurfaceScans(R.single_triangle(), 1.0, PIPE_K, PIPE_N, device=dev).get_uniform_and_surface_points(500)
    with pytest.raises(P.BadMeshException):
        P.SurfaceScans(R.single_triangle(), 1.0, PIPE_K, PIPE_N, device=dev).sample_sdf_near_surface(500)


def test_uniform_and_surface_points_and_the_bad_mesh():
    check_uniform_and_surface("cpu")


# ---- files ---------------------------------------------------------------------------------------------------------------------------------
def write_obj(path, vertices, faces, style="plain"):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("# test mesh\nmtllib none.mtl\n")
        for v in vertices:
            fh.write("v %.9g %.9g %.9g\n" % tuple(v))
        fh.write("vn 0 0 1\nvt 0 0\n")
        for f in faces:
            if style == "plain":
                fh.write("f " + " ".join("%d" % (i + 1) for i in f) + "\n")
            elif style == "slashes":
                fh.write("f " + " ".join("%d/1/1" % (i + 1) for i in f) + "\n")
            else:
                fh.write("f " + " ".join("%d//1" % (i - len(vertices)) for i in f) + "\n")


def test_load_obj_forms(tmp_path):
    v, f = R.mesh("box")
    for style in ("plain", "slashes", "negative"):
        path = str(tmp_path / style / "m.obj")
        write_obj(path, v, f, style)
        gv, gf = P.load_obj(path)
        np.testing.assert_allclose(gv, v, rtol=1e-8)
        np.testing.assert_array_equal(gf, f)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1)]
    path = str(tmp_path / "quads.obj")
    write_obj(path, v, quads)
    _, gf = P.load_obj(path)
    np.testing.assert_array_equal(gf, [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1)])
    # a pentagon with mixed forms on one line
    with open(path, "w") as fh:
        fh.write("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0.5 1.5 0\nv 0 1 0\nf 1 2/1 3//1 4/1/1 -1\n")
    gv, gf = P.load_obj(path)
    assert gv.shape == (5, 3)
    np.testing.assert_array_equal(gf, [(0, 1, 2), (0, 2, 3), (0, 3, 4)])


def test_scaling():
    v = np.array([[1.0, 2.0, 3.0], [5.0, 4.0, 3.5], [2.0, 2.5, 3.25]])
    cube = P.scale_to_unit_cube(v)
    assert np.allclose(cube.min(axis=0)[0], -1) and np.allclose(cube.max(axis=0)[0], 1) and np.allclose((cube.min(axis=0) + cube.max(axis=0)), 0)
    sphere = P.scale_to_unit_sphere(v)
    assert np.isclose(np.linalg.norm(sphere, axis=1).max(), 1) and np.allclose((sphere.min(axis=0) + sphere.max(axis=0)), 0)
    assert P.get_hash("data/shapenet/03001627/abc123/models/model_normalized.obj") == "abc123"


def test_command_line_writes_a_data_tree_the_loaders_read(tmp_path):
    models, data = str(tmp_path / "shapenet" / "0300"), str(tmp_path / "data")
    meshes = {"aaa": R.mesh("icosphere"), "bbb": R.single_triangle(), "ccc": R.mesh("torus")}
    for name, (v, f) in meshes.items():
        write_obj(os.path.join(models, name, "models", "model_normalized.obj"), v * 3.0 + 1.0, f)
    # a file that does not parse, in one batch with a good one: it costs that one model
    os.makedirs(os.path.join(models, "ddd", "models"))
    with open(os.path.join(models, "ddd", "models", "model_normalized.obj"), "w") as fh:
        fh.write("v 0 0 0\nv 1 0 zero\nf 1 2 9\n")
    argv = ["--models", models, "--dataset", "things", "--data", data, "--resolutions", "8", "16", "--uniform-and-surface", "--sdf-clouds",
            "--scan-count", str(PIPE_K), "--scan-resolution", str(PIPE_N), "--batch", "2", "--device", "cpu", "--cloud-size", "1000",
            "--sample-size", "1500"]
    assert P.main(argv) == 0
    root = os.path.join(data, "things")
    for res in (8, 16):
        ds = datasets.VoxelDataset.glob(os.path.join(root, "voxels_%d" % res, "**.npy"))
        # (the single triangle may or may not pass the voxel check: its field is unsigned up to the bias; the point sets decide)
        assert [os.path.basename(f) for f in ds.files if "bbb" not in f] == ["aaa.npy", "ccc.npy"]
        raw = np.load(ds.files[0])
        assert raw.shape == (res, res, res) and raw.dtype == np.float32 and (raw < 0).any()
        assert ds[0].shape == (res, res, res) and float(ds[0].abs().max()) <= 1.0
    assert sorted(os.listdir(os.path.join(root, "bad_meshes"))) == ["bbb"]
    assert not any("ddd" in f for _, _, files in os.walk(data) for f in files)
    assert sorted(os.listdir(os.path.join(root, "cloud"))) == ["aaa.npy", "ccc.npy"]
    assert sorted(os.listdir(os.path.join(root, "uniform"))) == sorted(os.listdir(os.path.join(root, "surface"))) == ["aaa.npy", "ccc.npy"]
    with open(os.path.join(root, "train.txt"), "w") as fh:
        fh.write("aaa\nccc\n")
    np.random.seed(0)
    uniform, surface = datasets.PointDataset.from_split(root, "train", num_points=64)[1]
    assert uniform.shape == surface.shape == (64, 4) and uniform.dtype == surface.dtype == torch.float32
    rows = np.load(os.path.join(root, "uniform", "aaa.npy"))
    assert rows.shape == (1500, 4) and rows.dtype == np.float32 and (np.linalg.norm(rows[:, :3], axis=1) < 1).all()
    cloud = np.load(os.path.join(root, "cloud", "ccc.npy"))
    assert cloud.shape == (1000, 4) and cloud.dtype == np.float32
    points, sdf, signs = datasets.load_sdf_clouds(data, device="cpu")
    assert points.shape == (2000, 3) and sdf.shape == (2000,) and points.dtype == sdf.dtype == torch.float32 and signs.shape == (2000,)
    assert signs.any() and not signs.all()
    np.testing.assert_array_equal(points[1000:].numpy(), cloud[:, :3])
    # the sphere was scaled to the unit sphere: its radius is 1, the SDF of the uniform points is |p| - 1 up to the facets (0.02) and
    # a sign that may be wrong within the bias of the surface (2 * 2 / N)
    assert np.abs(rows[:, 3] - (np.linalg.norm(rows[:, :3], axis=1) - 1)).max() < 0.02 + 4.0 / PIPE_N

    def snapshot():
        return {os.path.join(d, f): os.stat(os.path.join(d, f)).st_mtime_ns for d, _, files in os.walk(data) for f in files
                if not f.endswith(".to") and f != "train.txt"}

    before = snapshot()
    assert P.process_models(models, "things", data, (8, 16), True, True, PIPE_K, PIPE_N, 2, "cpu", 1000, 1500) == 0
    assert snapshot() == before


def test_reference_chair_if_present():
    path = os.path.join(ROOT, "..", "reference", "examples", "chair.obj")
    if not os.path.exists(path):
        pytest.skip("the reference's example mesh is not here")
    v, f = P.load_obj(path)
    assert len(f) > 100
    scans = P.SurfaceScans((P.scale_to_unit_cube(v), f), 3 ** 0.5, PIPE_K, PIPE_N, device="cpu")
    voxels = scans.get_voxels(16, check_result=True)
    assert P.check_voxels(voxels) is True and (voxels < 0).any()
