"""Inputs and checks of the distance-transform tests (K21), shared by the twin tier (tests/test_edt.py) and the GPU tier
(tests/test_gpu_edt.py).  References come from tests/edt_reference.py (float64, brute force over all sites), computed once per case.

THE BOUND.  u = 2^-24 is the unit roundoff of float32.  A pass computes, per candidate, d = (float)(p - q) * spacing (p - q is an
integer below 2^24 and converts exactly: ONE rounding) and fmaf(d, d, g) (ONE rounding); the first pass of a crossing family has
d = ((float)p - u_site) * spacing (TWO roundings).  A d with r roundings is d (1 + e)^r, its square d^2 (1 + e)^(2r); with g carrying
the relative error E of the pass before, fmaf(d, d, g) = (d^2 (1 + e)^(2r) + g (1 + E)) (1 + e): relative error at most
max(2r, E / u) + 1 units.  The minimum of values that each carry a relative error carries it too.  So
    voxels, any spacing:   2 + 1 = 3 after the first pass (g = 0), max(2, 3) + 1 = 4, then 5:          K_VOXELS = 5
    crossings:             4 + 1 = 5 after the crossing pass, max(2, 5) + 1 = 6, then 7:               K_CROSSINGS = 7
and |T32 - T64| <= k u T64, the first-order bound in the form the contract states it (the terms of second order, about 14 u^2 for
k = 7, are 2e-7 of the bound).  With unit spacing every candidate of `voxels` is an integer below 2^24: T32 == T64 exactly.  The
signed distance is the correctly rounded root: out == (float32)sqrt((float64)T32), bit for bit.  Nothing here is tuned on outputs."""
import functools
import os

import numpy as np
import torch

import edt_reference as R
from shapegan_amd import lib as L
from shapegan_amd import mesh, metrics, ops
from shapegan_amd import voxeldist as V

U = 2.0 ** -24
K_VOXELS, K_CROSSINGS = 5, 7
FORM_LDS, FORM_GLOBAL = L.abi.DEFINES["SG_EDT_FORM_LDS"], L.abi.DEFINES["SG_EDT_FORM_GLOBAL"]
ERR_ARG, ERR_WORKSPACE = -1, -3


def bound(k):
    return k * U


def t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)      # a copy: the cases are read-only


def noise(seed, shape):
    return np.clip(np.random.default_rng(seed).normal(0, 0.7, size=shape), -1, 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def threshold_shapes():
    """((D0, 32, 32), (D0 + 1, 32, 32)): the largest shape of the LDS form and the smallest of the global form with 32 x 32 planes,
    asked of sg_edt_form."""
    like = torch.zeros(1)
    d = 1
    while ops.edt_form((d + 1, 32, 32), like) == FORM_LDS:
        d += 1
    assert ops.edt_form((d, 32, 32), like) == FORM_LDS and ops.edt_form((d + 1, 32, 32), like) == FORM_GLOBAL
    return (d, 32, 32), (d + 1, 32, 32)


def _blobs(seed, shape, count=2):
    """A smooth field with a few small round regions below zero, plus a little noise: few sites and few crossings on a large grid."""
    rng = np.random.default_rng(seed)
    grid = np.full(shape, 1e9)
    axes = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    for _ in range(count):
        c = [rng.uniform(0.2, 0.8) * (n - 1) for n in shape]
        r = rng.uniform(2.5, 5.0)
        grid = np.minimum(grid, np.sqrt(sum((x - ci) ** 2 for x, ci in zip(axes, c))) - r)
    return np.clip(grid / 3.0 + rng.normal(0, 0.02, size=shape), -1, 1).astype(np.float32)


def _case(name):
    """(grids [S, D, H, W] float32, level, spacing)"""
    if name == "one-voxel":
        return np.array([-1.0, 1.0, -0.25], dtype=np.float32).reshape(3, 1, 1, 1), 0.0, 1.0
    if name == "one-line":
        g = np.array([[1, -1, -1, 0.5, 1, -0.25, 1], [1, 1, 1, 1, 1, 1, -1]], dtype=np.float32).reshape(2, 1, 7, 1)
        return g, 0.0, 1.0
    if name == "odd":                      # S = 3 with different content per grid
        return np.stack([noise(3 + i, (6, 5, 9)) for i in range(3)]), 0.125, 1.0
    if name == "odd-spaced":
        return np.stack([noise(7 + i, (6, 5, 9)) for i in range(2)]), 0.0, (0.3, 0.7, 1.1)
    if name == "wide":                     # W longer than a wave and no multiple of 64
        return np.stack([noise(11, (3, 4, 130)), _blobs(12, (3, 4, 130))]), 0.0, 1.0
    if name in ("lds-largest", "global-smallest"):      # a grid without sites between two others, in both forms
        shape = threshold_shapes()[0 if name == "lds-largest" else 1]
        return np.stack([_blobs(13, shape), np.ones(shape, dtype=np.float32), _blobs(14, shape, 3)]), 0.0, 2.0 / 32
    if name == "global-flat":              # the global form without a D pass, W no multiple of the workgroup
        return _blobs(15, (1, 190, 191), 6)[None], 0.0, (1.0, 0.5, 0.25)
    if name == "corner":                   # a single site in a corner: no early exit ever fires
        g = np.ones((2, 9, 10, 11), dtype=np.float32)
        g[0, 0, 0, 0] = -1.0
        g[1, 8, 9, 10] = -0.5
        return g, 0.0, 1.0
    if name == "last-planes":              # sites only on the last plane of each axis
        g = np.ones((1, 6, 7, 8), dtype=np.float32)
        g[0, -1], g[0, :, -1], g[0, :, :, -1] = -1.0, -1.0, -1.0
        return g, 0.0, 1.0
    if name == "checkerboard":             # all ties
        i, j, k = np.meshgrid(np.arange(6), np.arange(6), np.arange(7), indexing="ij")
        return np.where((i + j + k) % 2 == 0, -1.0, 1.0).astype(np.float32)[None], 0.0, 1.0
    if name == "anisotropic":              # the nearest site in index space is not the nearest in world space
        g = np.ones((1, 5, 5, 9), dtype=np.float32)
        g[0, 2, 3, 4] = -1.0               # one index step from (2, 2, 4): 2 world units
        g[0, 2, 2, 7] = -1.0               # three index steps: 1.5 world units
        return g, 0.0, (1.0, 2.0, 0.5)
    if name == "at-level":                 # a value exactly equal to the level: t = 0 (or 1) and the distance there is 0
        g = np.full((2, 4, 5, 6), -1.0, dtype=np.float32)
        g[0, 1, 2, 3] = 0.25
        g[1] = noise(21, (4, 5, 6))
        g[1, 2, 2, 2], g[1, 2, 2, 3] = 0.25, -0.5
        return g, 0.25, 1.0
    if name == "empty-between":            # a no-site grid between two others; S = 3
        return np.stack([noise(31, (6, 5, 9)), np.ones((6, 5, 9), dtype=np.float32), noise(32, (6, 5, 9))]), 0.0, 1.0
    raise KeyError(name)


CASES = ("one-voxel", "one-line", "odd", "odd-spaced", "wide", "lds-largest", "global-smallest", "global-flat", "corner", "last-planes",
         "checkerboard", "anisotropic", "at-level", "empty-between")
# what the dispatcher must choose: no form is left without a case
FORMS = {"lds-largest": FORM_LDS, "global-smallest": FORM_GLOBAL, "global-flat": FORM_GLOBAL, "odd": FORM_LDS, "wide": FORM_LDS}


@functools.lru_cache(maxsize=None)
def case(name):
    grids, level, spacing = _case(name)
    grids.setflags(write=False)
    return grids, level, spacing


@functools.lru_cache(maxsize=None)
def reference(name, sites):
    """Per grid of the case: (site coordinates [N, 3], T float64 [D, H, W])."""
    grids, level, spacing = case(name)
    out = []
    for g in grids:
        q = R.voxel_sites(g, level, True) if sites == "voxels" else R.crossing_sites(g, level)
        out.append((q, R.transform(g.shape, q, spacing)[0]))
    return out


def unit(spacing):
    return np.isscalar(spacing) and float(spacing) == 1.0


# ---- running ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def run(dev, name):
    """Everything the entry points make of a case: squared / nearest of `voxels` (inside), squared / closest of `crossings`, the same
    two without the optional output, the finished distances of both with and without the band."""
    grids, level, spacing = case(name)
    g = t(grids, dev)
    vsq, vidx = ops.edt_voxels(g, level, True, spacing, nearest=True)
    csq, cpos = ops.edt_crossings(g, level, spacing, closest=True)
    out = {"voxels": vsq, "nearest": vidx, "crossings": csq, "closest": cpos,
           "voxels-alone": ops.edt_voxels(g, level, True, spacing), "crossings-alone": ops.edt_crossings(g, level, spacing),
           "outside": ops.edt_voxels(g, level, False, spacing),
           "voxels-signed": ops.edt_finish(g, vsq, level), "crossings-signed": ops.edt_finish(g, csq, level),
           "voxels-root": ops.edt_finish(None, vsq),
           "crossings-band": ops.edt_finish(g, csq, level, 0.1, True)}
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_bitwise_equal(dev, other="cpu"):
    for name in CASES:
        a, b = run(dev, name), run(other, name)
        for key in a:
            assert a[key].shape == b[key].shape and np.array_equal(_bits(a[key]), _bits(b[key])), (name, key)


def _check_bound(name, what, got, ref, k):
    finite = np.isfinite(ref)
    assert np.array_equal(np.isposinf(got), ~finite), (name, what, "the voxels without a site")
    err = np.abs(got.astype(np.float64)[finite] - ref[finite])
    allowed = bound(k) * ref[finite]
    worst = float((err / np.maximum(ref[finite], 1e-300)).max() / U) if finite.any() else 0.0
    print("%s %s: worst relative error %.3g u (allowed %d u)" % (name, what, worst, k))
    assert (err <= allowed).all(), (name, what, worst)


def check_against_float64(dev, name):
    grids, level, spacing = case(name)
    out = run(dev, name)
    if name in FORMS:
        assert ops.edt_form(grids.shape[1:], torch.zeros(1, device=dev)) == FORMS[name]
    for s, g in enumerate(grids):
        # ---- voxels
        sites, T = reference(name, "voxels")[s]
        got = out["voxels"][s]
        if unit(spacing):
            assert np.array_equal(got.astype(np.float64), T), (name, "voxels with unit spacing are exact")
        else:
            _check_bound(name, "voxels", got, T, K_VOXELS)
        assert np.array_equal(_bits(out["voxels-alone"][s]), _bits(got))
        idx = out["nearest"][s]
        if len(sites):
            assert idx.min() >= 0 and idx.max() < g.size and (g.reshape(-1)[idx.reshape(-1)] < np.float32(level)).all(), (name, "nearest is a site")
            q = np.stack(np.unravel_index(idx, g.shape), axis=-1).astype(np.float64)
            attained = R.squared_to(g.shape, q, spacing)
            if unit(spacing):
                assert np.array_equal(attained, got.astype(np.float64)), (name, "nearest attains the distance")
            else:
                _check_bound(name, "nearest", got, attained, K_VOXELS)
        else:
            assert (idx == -1).all()
        # the other site set of `voxels`: the complement (on the large grids nearly every voxel: the brute force is left to the small)
        if g.size <= 4096:
            comp = R.transform(g.shape, R.voxel_sites(g, level, False), spacing)[0]
            if unit(spacing):
                assert np.array_equal(out["outside"][s].astype(np.float64), comp)
            else:
                _check_bound(name, "outside", out["outside"][s], comp, K_VOXELS)
        # ---- crossings
        sites, T = reference(name, "crossings")[s]
        got = out["crossings"][s]
        _check_bound(name, "crossings", got, T, K_CROSSINGS)
        assert np.array_equal(_bits(out["crossings-alone"][s]), _bits(got))
        pos = out["closest"][s]
        if len(sites):
            world = R.world_float32(sites, spacing)
            table = {row.tobytes(): i for i, row in enumerate(world)}
            which = np.array([table.get(row.tobytes(), -1) for row in pos.reshape(-1, 3)])
            assert (which >= 0).all(), (name, "closest is one of the crossings, bit for bit")
            attained = R.squared_to(g.shape, sites[which].reshape(g.shape + (3,)), spacing)
            _check_bound(name, "closest", got, attained, K_CROSSINGS)
        else:
            assert np.isnan(pos).all()
        # ---- finishing: the correctly rounded root, the sign of the input, the band
        sign = np.where(g < np.float32(level), -1.0, 1.0)
        for key in ("voxels", "crossings"):
            root = (sign * np.sqrt(out[key][s].astype(np.float64))).astype(np.float32)
            assert np.array_equal(_bits(out[key + "-signed"][s]), _bits(root)), (name, key, "signed")
        assert np.array_equal(_bits(out["voxels-root"][s]), _bits(np.sqrt(out["voxels"][s].astype(np.float64)).astype(np.float32)))
        band = R.finish(g, out["crossings"][s].astype(np.float64), level, 0.1, True).astype(np.float32)
        assert np.array_equal(_bits(out["crossings-band"][s]), _bits(band)), (name, "band")


def check_case_properties(dev):
    """What the cases were built for."""
    out = run(dev, "anisotropic")
    assert out["nearest"][0, 2, 2, 4] == (2 * 5 + 2) * 9 + 7 and out["voxels"][0, 2, 2, 4] == 2.25
    out, (grids, level, _) = run(dev, "at-level"), case("at-level")
    assert out["crossings"][0, 1, 2, 3] == 0.0 and out["crossings"][1, 2, 2, 2] == 0.0
    assert (out["crossings"][grids != np.float32(level)] > 0).all()
    out = run(dev, "corner")
    assert out["voxels"][0, 8, 9, 10] == 64 + 81 + 100 and out["voxels"][1, 0, 0, 0] == 64 + 81 + 100
    out = run(dev, "checkerboard")
    assert set(np.unique(out["crossings"][0])) == {0.25} and set(np.unique(out["voxels"][0])) == {0.0, 1.0}
    for name in ("empty-between", "lds-largest", "global-smallest"):
        out = run(dev, name)
        assert np.isposinf(out["voxels"][1]).all() and np.isposinf(out["crossings"][1]).all() and (out["nearest"][1] == -1).all()
        assert np.isnan(out["closest"][1]).all() and np.isposinf(out["crossings-signed"][1]).all()
        assert np.isfinite(out["voxels"][0]).all() and np.isfinite(out["crossings"][2]).all()
    out = run(dev, "one-voxel")
    assert out["voxels"].reshape(-1).tolist() == [0.0, np.inf, 0.0] and np.isposinf(out["crossings"]).all()
    assert out["voxels-signed"].reshape(-1).tolist() == [-0.0, np.inf, -0.0]


def check_batch_independence(dev):
    grids, level, spacing = case("odd")
    whole = run(dev, "odd")
    for s in range(grids.shape[0]):
        g = t(grids[s:s + 1], dev)
        sq, idx = ops.edt_voxels(g, level, True, spacing, nearest=True)
        csq, pos = ops.edt_crossings(g, level, spacing, closest=True)
        for got, key in ((sq, "voxels"), (idx, "nearest"), (csq, "crossings"), (pos, "closest")):
            assert np.array_equal(_bits(got.cpu().numpy()[0]), _bits(whole[key][s])), (s, key)


# ---- the definition --------------------------------------------------------------------------------------------------------------------
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edt_scipy.npz"))


def golden_masks():
    g = golden()
    for name in "abcdef":
        shape = tuple(int(n) for n in g["%s_shape" % name])
        mask = np.unpackbits(g["%s_bits" % name])[:int(np.prod(shape))].reshape(shape).astype(bool)
        yield name, mask, g["%s_unit" % name], g["%s_sampled" % name], tuple(float(x) for x in g["sampling"])


def check_reference_equals_golden():
    for name, mask, unit_out, sampled_out, sampling in golden_masks():
        grid = np.where(mask, 1.0, -1.0).astype(np.float32)      # scipy's sites are the zeros of the mask
        sites = R.voxel_sites(grid, 0.0, True)
        assert np.abs(np.sqrt(R.transform(mask.shape, sites, 1.0)[0]) - unit_out).max() <= 1e-12, name
        assert np.abs(np.sqrt(R.transform(mask.shape, sites, sampling)[0]) - sampled_out).max() <= 1e-12, name


def check_reference_equals_live_scipy(ndimage):
    rng = np.random.default_rng(5)
    for shape, density, sampling in (((5, 7, 4), 0.7, None), ((9, 9, 9), 0.95, (1.0, 2.0, 0.5)), ((1, 6, 3), 0.5, (0.25, 0.5, 4.0))):
        mask = rng.random(shape) < density
        sites = R.voxel_sites(np.where(mask, 1.0, -1.0), 0.0, True)
        ref = np.sqrt(R.transform(shape, sites, 1.0 if sampling is None else sampling)[0])
        assert np.abs(ref - ndimage.distance_transform_edt(mask, sampling=sampling)).max() <= 1e-12


def check_distance_transform_equals_golden(dev):
    """The public function on scipy's own inputs: exact squares and correctly rounded roots with unit sampling, the bound otherwise;
    the indices name a zero of the mask that attains the distance."""
    for name, mask, unit_out, sampled_out, sampling in golden_masks():
        dist, coords = V.distance_transform(t(mask, dev), return_indices=True)
        sq = V.distance_transform(t(mask, dev), squared=True).cpu().numpy().astype(np.float64)
        assert np.array_equal(sq, np.rint(unit_out ** 2)), name
        assert np.array_equal(dist.cpu().numpy(), np.sqrt(sq).astype(np.float32)), name
        c = coords.cpu().numpy()
        assert c.shape == (3,) + mask.shape and not mask[c[0], c[1], c[2]].any()
        assert np.array_equal(R.squared_to(mask.shape, np.moveaxis(c, 0, -1).astype(np.float64), 1.0), sq), name
        sampled = V.distance_transform(t(mask.astype(np.uint8), dev), spacing=sampling, squared=True).cpu().numpy()
        _check_bound(name, "sampled", sampled, sampled_out ** 2, K_VOXELS)      # the golden root squared again: float64, far below u


# ---- the crossings are marching cubes' vertices ------------------------------------------------------------------------------------------
def check_crossings_are_the_mesh_vertices(dev):
    for name in ("odd", "odd-spaced", "at-level", "wide"):
        grids, level, spacing = case(name)
        out = run(dev, name)
        sp = tuple(float(x) for x in R.spacing3(spacing))
        for s, g in enumerate(grids):
            batch = mesh.marching_cubes(t(g, dev), level=level, spacing=sp, origin=(0.0, 0.0, 0.0), pad=False)
            verts = batch.vertices.cpu().numpy()
            sites = R.crossing_sites(g, level)
            assert {r.tobytes() for r in verts} == {r.tobytes() for r in R.world_float32(sites, spacing)}, (name, s, "the same bits")
            assert {r.tobytes() for r in out["closest"][s].reshape(-1, 3)} <= {r.tobytes() for r in verts}
            # brute force over the mesh's own vertices.  With unit spacing a vertex's world position IS its index coordinate (u * 1.0f), so
            # the distances to the emitted vertices are held to the bound directly; with another spacing the vertex is the site rounded once
            # more (u * spacing in float32), which the bound does not cover: there the bit-equal vertex set above is the check
            if unit(spacing):
                _check_bound(name, "nearest vertex", out["crossings"][s], R.transform(g.shape, verts.astype(np.float64), 1.0)[0], K_CROSSINGS)


# ---- redistancing a sphere -------------------------------------------------------------------------------------------------------------
SPHERE_R, SPHERE_RADIUS = 24, 0.55
# measured with the float64 reference on sphere_grid(): the largest | sqrt(T64) - | |p| - r | | over the voxels outside the band.  It is
# the error of measuring to the nearest crossing instead of to the surface (the crossings are up to 1 / 12 apart, so a voxel just outside the
# band, 0.1 from the surface, can be sqrt(0.1^2 + 0.06^2) from the nearest of them), not a rounding error.  Measured: 0.02893.
SPHERE_SITE_ERROR = 2.9e-2


@functools.lru_cache(maxsize=None)
def sphere_grid():
    """(the clamped grid sdf / 0.1 in [-1, 1] as VoxelDataset holds it, the true distances |p| - r, the spacing)"""
    ax = (np.arange(SPHERE_R) + 0.5) / SPHERE_R * 2 - 1
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    sdf = np.sqrt(x * x + y * y + z * z) - SPHERE_RADIUS
    return (np.clip(sdf, -0.1, 0.1) / 0.1).astype(np.float32), sdf, 2.0 / SPHERE_R


@functools.lru_cache(maxsize=None)
def sphere_reference():
    grid, sdf, spacing = sphere_grid()
    sites = R.crossing_sites(grid, 0.0)
    T = R.transform(grid.shape, sites, spacing)[0]
    band = R.finish(grid, T, 0.0, 0.1, True) != R.finish(grid, T, 0.0, 0.1, False)
    return T, band, float(np.abs(np.sqrt(T) - np.abs(sdf))[~band].max())


def check_sphere_site_error_is_the_recorded_one():
    measured = sphere_reference()[2]
    print("sphere: site error %.4g (recorded %.4g)" % (measured, SPHERE_SITE_ERROR))
    assert SPHERE_SITE_ERROR / 2 <= measured <= SPHERE_SITE_ERROR


def check_redistance_recovers_a_sphere(dev):
    grid, sdf, spacing = sphere_grid()
    T, band, site_error = sphere_reference()
    out = V.redistance_grids(t(grid, dev)).cpu().numpy().astype(np.float64)      # the defaults: spacing 2 / R, value_scale 0.1, keep_band
    assert abs(sdf).max() > 0.9 and np.abs(grid).max() == 1.0 and (~band).sum() > band.sum()
    # |out - sdf| <= |out - s sqrt(T64)| + |sqrt(T64) - |sdf||: the rounding of T (the root halves it at least) and of the root, and
    # the measured site error
    allowed = site_error + (bound(K_CROSSINGS) + U) * np.sqrt(T)
    err = np.abs(out - sdf)
    print("sphere: worst error outside the band %.4g, inside it %.4g" % (err[~band].max(), err[band].max()))
    assert (err[~band] <= allowed[~band]).all()
    assert np.array_equal(out[band].astype(np.float32), (grid[band] * np.float32(0.1)).astype(np.float32))
    assert (np.sign(out) == np.where(grid < 0, -1, 1)).all()


def check_offset_moves_a_sphere(dev):
    """offset_grids and then meshing at 0, and marching_cubes(level=, redistance=True): the vertices lie on the sphere of radius
    r + distance to within the recorded site error (1e-6 for the float32 roundings of the distances and of the vertex positions)."""
    grid, sdf, spacing = sphere_grid()
    site_error = sphere_reference()[2]
    distance = 0.2                                                     # twice the truncation: the clamped grid is flat there
    origin = -1 + spacing / 2
    moved = V.offset_grids(t(grid, dev), distance)
    a = mesh.marching_cubes(moved, level=0.0, spacing=spacing, origin=origin, pad=False)
    b = mesh.marching_cubes(t(grid, dev), level=distance / 0.1, spacing=spacing, origin=origin, pad=False, redistance=True)
    plain = mesh.marching_cubes(t(grid, dev), level=distance / 0.1, spacing=spacing, origin=origin, pad=False)
    assert plain.vertices.shape[0] == 0                                # without redistancing there is no such level
    for batch in (a, b):
        radius = batch.vertices.cpu().numpy().astype(np.float64)
        radius = np.sqrt((radius * radius).sum(axis=1))
        assert len(radius) > 1000
        err = np.abs(radius - (SPHERE_RADIUS + distance))
        print("offset sphere: worst vertex error %.4g (allowed %.4g)" % (err.max(), site_error + 1e-6))
        assert err.max() <= site_error + 1e-6


# ---- the public layer ------------------------------------------------------------------------------------------------------------------
def check_occupancy_to_sdf(dev):
    grid, sdf, spacing = sphere_grid()
    occupancy = sdf < 0
    out = V.occupancy_to_sdf(t(occupancy, dev), clamp=0.1).cpu().numpy()
    assert out.min() == -1.0 and out.max() == 1.0 and ((out < 0) == occupancy).all() and (out != 0).all()
    raw = V.occupancy_to_sdf(t(occupancy, dev)).cpu().numpy()
    g = np.where(occupancy, -0.5, 0.5).astype(np.float32)
    sites = R.crossing_sites(g, 0.0)
    assert (sites * 2 == np.rint(sites * 2)).all() and len(sites)      # edge midpoints: t = 0.5 exactly
    T = R.transform(g.shape, sites, spacing)[0]
    _check_bound("occupancy", "squared", (raw.astype(np.float64) ** 2).astype(np.float64), T, K_CROSSINGS + 2)      # root and square
    assert np.array_equal(np.clip(raw, -0.1, 0.1) / np.float32(0.1), out)


def check_hooks_off_change_nothing(dev, monkeypatch):
    grid = t(sphere_grid()[0], dev)
    a = mesh.marching_cubes(grid, level=0.25, spacing=2 / SPHERE_R, origin=-1)
    b = mesh.marching_cubes(grid, level=0.25, spacing=2 / SPHERE_R, origin=-1, redistance=False)
    called = []
    monkeypatch.setattr(V, "redistance_grids", lambda *args, **kw: called.append(1))
    c = mesh.marching_cubes(grid, level=0.25, spacing=2 / SPHERE_R, origin=-1)
    for x in (b, c):
        assert torch.equal(a.vertices, x.vertices) and torch.equal(a.faces, x.faces) and torch.equal(a.normals, x.normals)
    monkeypatch.setattr(metrics, "device", torch.device(dev))
    grids = torch.stack([grid, -grid.flip(0)])
    torch.manual_seed(3)
    p = metrics.sample_from_voxels(grids, 64)
    torch.manual_seed(3)
    q = metrics.sample_from_voxels(grids, 64, redistance=False)
    assert np.array_equal(p, q) and not called


def check_sample_from_voxels_redistance(dev, monkeypatch):
    monkeypatch.setattr(metrics, "device", torch.device(dev))
    seen = []
    real = V.redistance_grids
    monkeypatch.setattr(V, "redistance_grids", lambda *args, **kw: seen.append(1) or real(*args, **kw))
    grids = torch.stack([t(sphere_grid()[0], dev)] * 2)
    p = metrics.sample_from_voxels(grids, 128, redistance=True)
    assert seen and p.shape == (2, 128, 3) and np.isfinite(p).all()


def check_voxel_dataset_occupancy(dev, tmp_path):
    from shapegan_amd import datasets
    grid, sdf, _ = sphere_grid()
    files = []
    for i, r in enumerate((0.0, 0.1)):
        files.append(str(tmp_path / ("%d.npy" % i)))
        np.save(files[-1], (sdf < r).astype(np.float32))
    expected = torch.stack([V.occupancy_to_sdf(t(np.load(f), dev), clamp=0.1) for f in files])
    if dev == "cpu":      # resident() and stream() pin host memory, which takes a GPU: the step they add, on its own
        batch = t(np.stack([np.load(f) for f in files]), dev)
        assert datasets.VoxelDataset(files, occupancy=True)._distances(batch) is batch
        assert torch.equal(ops.voxel_prepare(batch, 0.1, 0.1), expected)
        untouched = t(np.stack([np.load(f) for f in files]), dev)
        assert torch.equal(datasets.VoxelDataset(files)._distances(untouched.clone()), untouched)
        return
    got = datasets.VoxelDataset(files, occupancy=True).resident(device=dev).data
    assert torch.equal(got, expected) and got.min() == -1 and got.max() == 1
    plain = datasets.VoxelDataset(files).resident(device=dev).data      # the flag off: the files as they are, clamped and rescaled
    assert torch.equal(plain, t(np.stack([np.load(f) for f in files]), dev).clamp(-0.1, 0.1) / 0.1)
    torch.manual_seed(0)
    batches = list(datasets.VoxelDataset(files, occupancy=True).stream(2, device=dev, shuffle=False))
    assert len(batches) == 1 and torch.equal(batches[0], expected)


def check_binvox_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    dims = (3, 4, 5)
    voxels = rng.random(dims) < 0.4
    voxels[0, 0, :] = True                                              # a run longer than one pair would be at 255: here a few pairs
    flat = voxels.transpose(0, 2, 1).reshape(-1)                        # x slowest, then z, then y
    pairs, i = bytearray(), 0
    while i < len(flat):
        j = i
        while j < len(flat) and flat[j] == flat[i] and j - i < 3:      # short runs: several pairs per run
            j += 1
        pairs += bytes((int(flat[i]), j - i))
        i = j
    path = tmp_path / "tiny.binvox"
    path.write_bytes(b"#binvox 1\ndim 3 4 5\ntranslate -0.5 0.25 1\nscale 2.5\ndata\n" + bytes(pairs))
    got, translate, scale = V.load_binvox(str(path))
    assert got.dtype == torch.bool and tuple(got.shape) == dims and np.array_equal(got.numpy(), voxels)
    assert translate == (-0.5, 0.25, 1.0) and scale == 2.5
    sdf = V.occupancy_to_sdf(got, spacing=scale / 5)
    assert ((sdf < 0).numpy() == voxels).all()
    (tmp_path / "bad.binvox").write_bytes(b"#binvox 1\ndim 3 4 5\ndata\n\x01\x05")
    try:
        V.load_binvox(str(tmp_path / "bad.binvox"))
    except ValueError as e:
        assert "holds 5 voxels" in str(e)
    else:
        raise AssertionError("a short data section was accepted")


def check_input_forms(dev):
    grids, level, spacing = case("odd")
    ref = V.redistance_grids(t(grids, dev), level, 1.0, 1.0, False)
    assert ref.dtype == torch.float32 and ref.device.type == torch.device(dev).type and tuple(ref.shape) == grids.shape
    assert torch.equal(V.redistance_grids(t(grids[1], dev), level, 1.0, 1.0, False), ref[1])                       # one grid
    assert torch.equal(V.redistance_grids(t(grids.astype(np.float64), dev), level, 1.0, 1.0, False), ref)          # another dtype
    swapped = t(np.ascontiguousarray(grids.transpose(0, 3, 2, 1)), dev).permute(0, 3, 2, 1)
    assert not swapped.is_contiguous() and torch.equal(V.redistance_grids(swapped, level, 1.0, 1.0, False), ref)   # not contiguous
    if dev == "cpu":
        assert torch.equal(V.redistance_grids(grids.copy(), level, 1.0, 1.0, False), ref)                          # numpy
    sdf, where = V.redistance_grids(t(grids[0], dev), level, 1.0, 1.0, False, return_closest=True)
    assert tuple(where.shape) == grids.shape[1:] + (3,) and torch.equal(sdf, ref[0])
    mask = t(grids < 0, dev)
    d = V.distance_transform(mask)
    assert torch.equal(d, V.distance_transform(mask.to(torch.int64))) and torch.equal(d, V.distance_transform(mask.float()))
    old = V._MAX_ELEMENTS
    try:
        V._MAX_ELEMENTS = 2 * grids[0].size      # the batch is split in two calls
        assert torch.equal(V.redistance_grids(t(grids, dev), level, 1.0, 1.0, False), ref)
        both = V.distance_transform(mask, return_indices=True)
    finally:
        V._MAX_ELEMENTS = old
    whole = V.distance_transform(mask, return_indices=True)
    assert torch.equal(both[0], whole[0]) and torch.equal(both[1], whole[1])


def check_empty(dev):
    g = torch.zeros((0, 4, 5, 6), device=dev)
    sq, idx = ops.edt_voxels(g, nearest=True)
    csq, pos = ops.edt_crossings(g, closest=True)
    assert tuple(sq.shape) == (0, 4, 5, 6) == tuple(idx.shape) == tuple(csq.shape) and tuple(pos.shape) == (0, 4, 5, 6, 3)
    assert tuple(ops.edt_finish(g, sq).shape) == (0, 4, 5, 6)


def check_argument_errors(dev):
    import pytest
    g = torch.zeros((1, 4, 5, 6), device=dev)
    for bad in (0.0, -1.0, float("inf"), float("nan"), (1.0, 2.0)):
        with pytest.raises(ValueError, match="spacing"):
            ops.edt_voxels(g, spacing=bad)
        with pytest.raises(ValueError, match="spacing"):
            ops.edt_crossings(g, spacing=bad)
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.edt_voxels(g.double())
    with pytest.raises(ValueError, match="differentiable"):
        V.redistance_grids(torch.zeros((4, 5, 6), device=dev, requires_grad=True))
    with pytest.raises(ValueError, match="differentiable"):
        V.distance_transform(torch.zeros((4, 5, 6), device=dev, requires_grad=True))
    with pytest.raises(ValueError, match="1 to %d" % V.MAX_AXIS):
        V.redistance_grids(torch.zeros((1, 1, V.MAX_AXIS + 1), device=dev))
    with pytest.raises(ValueError, match="expected"):
        V.redistance_grids(torch.zeros((5, 6), device=dev))
    with pytest.raises(ValueError, match="shape and device"):
        ops.edt_finish(g, torch.zeros((1, 4, 5, 7), device=dev))
    with pytest.raises(ValueError, match="keep_band needs the grids"):
        ops.edt_finish(None, g, keep_band=True)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.edt_crossings(g, level=float("nan"))
    like = torch.zeros(1, device=dev)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.edt_form((1, 1, V.MAX_AXIS + 1), like)
    assert ops.edt_form((1, 1, V.MAX_AXIS), like) == FORM_LDS


def check_short_workspace(dev):
    """One byte short: SG_ERR_WORKSPACE and the outputs untouched, in both forms and with the optional outputs."""
    lib = ops._lib()
    for shape, closest in (((6, 5, 9), True), (threshold_shapes()[1], False), (threshold_shapes()[1], True)):
        for sites in (ops.EDT_VOXELS, ops.EDT_CROSSINGS):
            need = lib.sg_edt_workspace_bytes(sites, 2, *shape, int(closest))
            if need == 0:
                assert sites == ops.EDT_VOXELS and ops.edt_form(shape, torch.zeros(1, device=dev)) == FORM_LDS
                continue
            g = t(np.stack([noise(1, shape), noise(2, shape)]), dev)
            squared = torch.full((2,) + shape, -7.0, device=dev)
            extra = (torch.full((2,) + shape, -7, dtype=torch.int32, device=dev) if sites == ops.EDT_VOXELS
                     else torch.full((2,) + shape + (3,), -7.0, device=dev)) if closest else None
            ws = torch.zeros(need, dtype=torch.uint8, device=dev)
            for nbytes, expected in ((need - 1, ERR_WORKSPACE), (need, 0)):
                try:
                    L.note_device(g)
                    if sites == ops.EDT_VOXELS:
                        rc = lib.sg_edt_voxels(ops.ptr(g), 2, *shape, 0.0, 1, 1.0, 1.0, 1.0, ops.ptr(squared), ops.ptr(extra), ops.ptr(ws), nbytes,
                                               ops.stream())
                    else:
                        rc = lib.sg_edt_crossings(ops.ptr(g), 2, *shape, 0.0, 1.0, 1.0, 1.0, ops.ptr(squared), ops.ptr(extra), ops.ptr(ws), nbytes,
                                                  ops.stream())
                finally:
                    L.reset_call_state()
                assert rc == expected, (shape, sites, nbytes, rc)
                untouched = bool((squared == -7).all()) and (extra is None or bool((extra == -7).all()))
                assert untouched == (expected != 0)
