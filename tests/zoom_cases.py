"""Inputs and checks of the voxel-zoom tests (K20), shared by the twin tier (tests/test_zoom.py) and the GPU tier
(tests/test_gpu_zoom.py).  References come from tests/zoom_reference.py (float64, numpy only), computed once per case and shared.

Inputs are noise clamped to [-1, 1].  The tolerance is not tuned to the kernels: tests/zoom_reference.py run in numpy float32 over ZOOM_CASES
and SAMPLE_CASES below differs from its float64 self by at most F32_VALUE_ERROR (zoom outputs and sample values) and F32_GRADIENT_ERROR
(sample gradients), both measured with max|g| <= 1; the tests allow MARGIN = 4 times that, times max|g| — the margin because the device
contracts to fmaf where numpy rounds twice, and sums the 64 taps in another order than numpy's tensordot."""
import functools

import numpy as np
import torch

import zoom_reference as R
from shapegan_amd import lib as L
from shapegan_amd import ops
from shapegan_amd import voxelzoom as V

F32_VALUE_ERROR = 1.11e-6       # measured: 1.10e-6 over ZOOM_CASES (both orders), 6.4e-7 over SAMPLE_CASES
F32_GRADIENT_ERROR = 2.2e-6     # measured: 2.19e-6 over SAMPLE_CASES
MARGIN = 4
ERR_ARG = -1
TD, TH, TW = V.TILE
FORM_LDS, FORM_GLOBAL = L.abi.DEFINES["SG_SPLINE_FORM_LDS"], L.abi.DEFINES["SG_SPLINE_FORM_GLOBAL"]


def _short_axes():
    """Axis lengths 1, 2, 3 and 4 in every position of (5, 6, 7), each zoomed to (11, 9, 13)."""
    out = []
    for length in (1, 2, 3, 4):
        for pos in range(3):
            shape = [5, 6, 7]
            shape[pos] = length
            out.append((tuple(shape), (11, 9, 13)))
    return out


# (input shape, output size)
ZOOM_CASES = (
    # the golden shapes
    [((5, 7, 4), (15, 21, 12)), ((8, 8, 8), (16, 16, 16)), ((2, 3, 4), (8, 12, 16)), ((9, 9, 9), (22, 22, 22))]
    + _short_axes()
    # output lengths: 1, shorter than the input, the tile, the tile - 1 and + 1 on every axis, more than one tile on every axis
    + [((6, 5, 9), (1, 1, 1)), ((6, 5, 9), (4, 3, 5)), ((6, 5, 9), (TD, TH, TW)), ((6, 5, 9), (TD - 1, TH + 1, TW - 1)),
       ((6, 5, 9), (TD + 1, TH - 1, TW + 1)), ((6, 5, 9), (1, TH + 1, TW + 1)), ((4, 4, 30), (2 * TD + 3, 2 * TH + 1, 2 * TW + 5)),
       ((1, 1, 1), (3, 1, 2)), ((7, 7, 7), (7, 7, 7))]
    # the prefilter's two forms, at the threshold the header names: 32^3 is held in LDS, 40 x 32 x 32 goes through global memory;
    # a flat grid that goes through global memory without a D pass; the zoom's two forms
    + [((32, 32, 32), (33, 16, 70)), ((40, 32, 32), (41, 33, 66)), ((40, 32, 32), (8, 8, 8)), ((32, 32, 32), (3, 3, 3)),
       ((1, 192, 191), (1, 9, 65)), ((40, 1, 1000), (9, 1, 63))])

# what the dispatchers must choose on the cases above (prefilter form, zoom form): no form is left without a case
FORMS = {((32, 32, 32), (33, 16, 70)): (FORM_LDS, FORM_LDS), ((40, 32, 32), (41, 33, 66)): (FORM_GLOBAL, FORM_LDS),
         ((40, 32, 32), (8, 8, 8)): (FORM_GLOBAL, FORM_GLOBAL), ((32, 32, 32), (3, 3, 3)): (FORM_LDS, FORM_GLOBAL),
         ((1, 192, 191), (1, 9, 65)): (FORM_GLOBAL, FORM_GLOBAL), ((40, 1, 1000), (9, 1, 63)): (FORM_GLOBAL, FORM_GLOBAL),
         ((6, 5, 9), (4, 3, 5)): (FORM_LDS, FORM_LDS), ((7, 7, 7), (7, 7, 7)): (FORM_LDS, FORM_LDS)}

SAMPLE_CASES = [(6, 5, 7), (1, 4, 3), (3, 1, 4), (4, 3, 1), (2, 2, 2), (1, 1, 1), (3, 3, 3), (32, 32, 32), (40, 32, 32)]


def noise(seed, shape):
    return np.clip(np.random.default_rng(seed).normal(0, 0.7, size=shape), -1, 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def grid(shape):
    return noise(sum(shape) * 31 + shape[0], shape)


@functools.lru_cache(maxsize=None)
def reference_zoom(shape, size, order):
    return R.zoom(grid(shape), size, order)


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def tolerance(g, base=F32_VALUE_ERROR):
    return MARGIN * base * float(np.abs(g).max())


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zoom_scipy.npz"))


def check_reference_equals_golden():
    g = golden()
    for name in "abcde":
        x, factor, order, out = g["zoom_%s_in" % name], float(g["zoom_%s_factor" % name]), int(g["zoom_%s_order" % name]), g["zoom_%s_out" % name]
        assert R.zoom_size(x.shape, factor) == out.shape == V.zoom_size(x.shape, factor)
        assert np.abs(R.zoom(x, out.shape, order) - out).max() <= 1e-12
    values, _ = R.sample(g["sample_in"], g["sample_points"])
    assert np.abs(values - g["sample_out"]).max() <= 1e-12


def check_reference_equals_live_scipy(ndimage):
    rng = np.random.default_rng(9)
    for shape, factor, order in (((5, 7, 4), 3, 3), ((8, 8, 8), 2, 3), ((2, 3, 4), 4, 3), ((9, 9, 9), 2.5, 3), ((5, 7, 4), 3, 1), ((16, 16, 16), 2.5, 3)):
        x = np.clip(rng.normal(0, 0.7, size=shape), -1, 1)
        out = ndimage.zoom(x, factor, order=order)
        assert np.abs(R.zoom(x, out.shape, order) - out).max() <= 1e-12
    x = np.clip(rng.normal(0, 0.7, size=(6, 5, 7)), -1, 1)
    p = rng.uniform(0, 1, size=(200, 3)) * (np.array(x.shape) - 1)      # in-domain points only: outside, the header's rule stands
    assert np.abs(R.sample(x, p)[0] - ndimage.map_coordinates(x, p.T, order=3, mode="constant", cval=1.0)).max() <= 1e-12


def measure_float32_reference():
    """The figures behind F32_VALUE_ERROR and F32_GRADIENT_ERROR (printed by test_zoom.py::test_the_tolerance_is_the_measured_one)."""
    value, gradient = 0.0, 0.0
    for shape, size in ZOOM_CASES:
        for order in (3, 1):
            value = max(value, float(np.abs(R.zoom(grid(shape), size, order, np.float32) - reference_zoom(shape, size, order)).max()))
    sample_value = 0.0
    for shape in SAMPLE_CASES:
        pts = sample_points(shape)
        v32, g32 = R.sample(grid(shape), pts, outside=-3.5, dtype=np.float32)
        v64, g64 = reference_sample(shape)
        sample_value = max(sample_value, float(np.abs(v32 - v64).max()))
        gradient = max(gradient, float(np.abs(g32 - g64).max()))
    return value, sample_value, gradient


# ---- zoom ------------------------------------------------------------------------------------------------------------------------------
def run_zoom(dev, shape, size, order):
    g = t(grid(shape)[None], dev)
    c = ops.spline_prefilter(g) if order == 3 else g
    return c, ops.spline_zoom(c, size, order)


def check_zoom_against_float64(dev, shape, size):
    if (shape, size) in FORMS:
        like = torch.zeros(1, device=dev)
        assert (ops.spline_prefilter_form(shape, like), ops.spline_zoom_form(shape, size, like)) == FORMS[(shape, size)]
    for order in (3, 1):
        out = run_zoom(dev, shape, size, order)[1].cpu().numpy()[0]
        ref = reference_zoom(shape, size, order)
        err = float(np.abs(out - ref).max())
        print("%s -> %s order %d: error %.3g (allowed %.3g)" % (shape, size, order, err, tolerance(grid(shape))))
        assert out.shape == tuple(size) and err <= tolerance(grid(shape))
        public = V.zoom_grids(t(grid(shape), dev), size=size, order=order)
        assert torch.equal(public.cpu(), torch.from_numpy(out))


def zoom_outputs(dev):
    """Everything the prefilter and the zoom make on ZOOM_CASES, for the GPU-equals-twin comparison."""
    out = []
    for shape, size in ZOOM_CASES:
        for order in (3, 1):
            c, z = run_zoom(dev, shape, size, order)
            out += [c.cpu().numpy(), z.cpu().numpy()]
    return out


def check_bitwise_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype == np.float32
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


# ---- sample ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sample_points(shape):
    rng = np.random.default_rng(sum(shape))
    top = np.array(shape, dtype=np.float64) - 1
    inside = rng.uniform(0, 1, size=(257, 3)) * top
    nodes = np.floor(rng.uniform(0, 1, size=(40, 3)) * (top + 1)).clip(0, top)
    faces = rng.uniform(0, 1, size=(30, 3)) * top
    faces[np.arange(30), np.arange(30) % 3] = top[np.arange(30) % 3]                  # x = n - 1 exactly: inside
    corners = np.array([[0, 0, 0], top, [top[0], 0, top[2]]])
    beyond = rng.uniform(0, 1, size=(12, 3)) * top
    beyond[np.arange(6), np.arange(6) % 3] = top[np.arange(6) % 3] + 1e-3             # just outside, above and below
    beyond[6 + np.arange(6), np.arange(6) % 3] = -1e-3
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e9, 0, 0]])
    pts = np.concatenate([inside, nodes, faces, corners, beyond, odd]).astype(np.float32)
    return pts, len(inside) + len(nodes) + len(faces) + len(corners)


def sample_points(shape):
    return _sample_points(shape)[0]


@functools.lru_cache(maxsize=None)
def reference_sample(shape):
    return R.sample(grid(shape), sample_points(shape).astype(np.float64), outside=-3.5)


def run_sample(dev, shape, gradient=True):
    g, p = t(grid(shape)[None], dev), t(sample_points(shape)[None], dev)
    out = ops.spline_sample(ops.spline_prefilter(g), p, gradient, outside=-3.5)
    return tuple(x.cpu().numpy()[0] for x in (out if gradient else (out,)))


def check_sample_against_float64(dev, shape):
    values, grad = run_sample(dev, shape)
    ref_v, ref_g = reference_sample(shape)
    pts, n_inside = _sample_points(shape)
    assert (values[n_inside:] == np.float32(-3.5)).all() and (grad[n_inside:] == 0).all()      # outside: the caller's value, no gradient
    assert (ref_v[n_inside:] == -3.5).all() and (ref_v[:n_inside] != -3.5).all()
    err_v, err_g = float(np.abs(values - ref_v).max()), float(np.abs(grad - ref_g).max())
    print("%s: value error %.3g (allowed %.3g), gradient error %.3g (allowed %.3g)"
          % (shape, err_v, tolerance(grid(shape)), err_g, tolerance(grid(shape), F32_GRADIENT_ERROR)))
    assert err_v <= tolerance(grid(shape)) and err_g <= tolerance(grid(shape), F32_GRADIENT_ERROR)
    assert np.array_equal(run_sample(dev, shape, gradient=False)[0].view(np.int32), values.view(np.int32))
    public = V.sample_grids(t(grid(shape), dev), t(pts, dev), gradient=True, outside=-3.5)
    assert np.array_equal(public[0].cpu().numpy().view(np.int32), values.view(np.int32)) and public[1].shape == (len(pts), 3)


def sample_outputs(dev):
    out = []
    for shape in SAMPLE_CASES:
        out += list(run_sample(dev, shape))
    return out


# ---- properties ------------------------------------------------------------------------------------------------------------------------
def check_interpolation(dev):
    """(N - 1) a multiple of (n - 1): the outputs at the nodes are the inputs."""
    for n, N in ((5, 9), (5, 17), (4, 10)):
        shape, size = (n, n, n), (N, N, N)
        out = V.zoom_grids(t(grid(shape), dev), size=size).cpu().numpy()
        step = (N - 1) // (n - 1)
        err = float(np.abs(out[::step, ::step, ::step] - grid(shape)).max())
        print("%d -> %d: error at the nodes %.3g (allowed %.3g)" % (n, N, err, tolerance(grid(shape))))
        assert err <= tolerance(grid(shape))


def check_constant(dev):
    """A constant grid gives that constant within 4 ulp everywhere, sizes 1 to 9, up- and downscaled, values and samples."""
    for value in (1.0, 0.75, -0.3):
        c = np.float32(value)
        for n in range(1, 10):
            g = t(np.full((n, n, n), c, np.float32), dev)
            out = V.zoom_grids(g, size=(2 * n + 1, n + 3, max(1, n - 1))).cpu().numpy().astype(np.float64)
            pts = t((np.random.default_rng(n).uniform(0, 1, size=(50, 3)) * (n - 1)).astype(np.float32), dev)
            sampled = V.sample_grids(g, pts).cpu().numpy().astype(np.float64)
            ulp = float(np.spacing(np.abs(c)))
            assert np.abs(out - float(c)).max() <= 4 * ulp and np.abs(sampled - float(c)).max() <= 4 * ulp


def check_gradient_is_the_derivative(dev):
    """The gradient equals central differences of the float64 reference's own values."""
    shape = (6, 5, 7)
    rng = np.random.default_rng(4)
    pts = (0.25 + rng.uniform(0, 1, size=(100, 3)) * (np.array(shape) - 1.5)).astype(np.float32)      # h away from the faces
    _, grad = V.sample_grids(t(grid(shape), dev), t(pts, dev), gradient=True)
    grad = grad.cpu().numpy()
    h = 1e-4
    c = R.prefilter(grid(shape))
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        diff = (R.sample(grid(shape), pts.astype(np.float64) + e, coefficients=c)[0] - R.sample(grid(shape), pts.astype(np.float64) - e, coefficients=c)[0]) / (2 * h)
        assert np.abs(grad[:, a] - diff).max() <= tolerance(grid(shape), F32_GRADIENT_ERROR) + 1e-7      # + the h^2 term of the difference


def check_faces_and_outside(dev):
    shape = (6, 5, 7)
    g = t(grid(shape), dev)
    on = np.array([[5, 2.5, 3], [2, 4, 3.25], [1.5, 2, 6], [5, 4, 6], [0, 0, 0]], np.float32)
    off = on.copy()
    off[0, 0] += 1e-3
    off[1, 1] += 1e-3
    off[2, 2] += 1e-3
    off[3] += 1e-3
    off[4, 1] = -1e-3
    v_on, g_on = V.sample_grids(g, t(on, dev), gradient=True, outside=7.0)
    v_off, g_off = V.sample_grids(g, t(off, dev), gradient=True, outside=7.0)
    ref, ref_g = R.sample(grid(shape), on.astype(np.float64), outside=7.0)
    assert (v_on.cpu().numpy() != 7.0).all() and np.abs(v_on.cpu().numpy() - ref).max() <= tolerance(grid(shape))
    assert np.abs(v_on.cpu().numpy()[3:] - np.array([grid(shape)[5, 4, 6], grid(shape)[0, 0, 0]])).max() <= tolerance(grid(shape))
    assert np.abs(g_on.cpu().numpy() - ref_g).max() <= tolerance(grid(shape), F32_GRADIENT_ERROR) and (g_on.cpu().numpy()[:3] != 0).any(axis=1).all()
    assert (v_off.cpu().numpy() == 7.0).all() and (g_off.cpu().numpy() == 0).all()


def check_batch_independence(dev):
    """S = 3: each grid equals its S = 1 call bit for bit, in every form."""
    for shape, size in (((6, 5, 9), (TD + 1, TH - 1, TW + 1)), ((40, 32, 32), (8, 8, 8)), ((32, 32, 32), (9, 5, 65))):
        grids = np.stack([noise(100 + i, shape) for i in range(3)])
        pts = np.stack([sample_points(shape)] * 3)
        pts[1] = pts[1][::-1]
        c = ops.spline_prefilter(t(grids, dev))
        z3, z1 = ops.spline_zoom(c, size, 3), ops.spline_zoom(t(grids, dev), size, 1)
        v, g = ops.spline_sample(c, t(pts, dev), True, 2.0)
        for i in range(3):
            ci = ops.spline_prefilter(t(grids[i:i + 1], dev))
            vi, gi = ops.spline_sample(ci, t(pts[i:i + 1], dev), True, 2.0)
            alone = [ci, ops.spline_zoom(ci, size, 3), ops.spline_zoom(t(grids[i:i + 1], dev), size, 1), vi, gi]
            check_bitwise_equal([x[i:i + 1].cpu().numpy() for x in (c, z3, z1, v, g)], [x.cpu().numpy() for x in alone])


def check_empty(dev):
    none = torch.zeros((0, 4, 5, 6), device=dev)
    assert V.spline_coefficients(none).shape == (0, 4, 5, 6) and V.zoom_grids(none, zoom=2).shape == (0, 8, 10, 12)
    assert V.sample_grids(none, torch.zeros((0, 7, 3), device=dev)).shape == (0, 7)
    g = t(grid((4, 3, 5))[None], dev)
    v, grad = V.sample_grids(g, torch.zeros((1, 0, 3), device=dev), gradient=True)
    assert v.shape == (1, 0) and grad.shape == (1, 0, 3)
    # the raw entries: 0, and nothing launched (a NULL pointer would fault otherwise)
    lib = L.load()
    for call in (lambda: lib.sg_spline_prefilter(None, 0, 4, 5, 6, None, L.stream()),
                 lambda: lib.sg_spline_zoom(None, 0, 4, 5, 6, 8, 10, 12, 3, None, L.stream()),
                 lambda: lib.sg_spline_sample(None, 0, 4, 5, 6, None, 7, 1.0, None, None, L.stream()),
                 lambda: lib.sg_spline_sample(L.ptr(g), 1, 4, 3, 5, None, 0, 1.0, None, None, L.stream())):
        L.note_device(g)
        try:
            assert call() == 0
        finally:
            L.reset_call_state()


def _raises(kind, fn):
    try:
        fn()
    except kind:
        return
    raise AssertionError("%s was not raised" % kind.__name__)


def check_argument_errors(dev):
    g = t(grid((4, 3, 5))[None], dev)
    p = torch.zeros((1, 2, 3), device=dev)
    # from Python: wrong rank, a zero-length axis, order 2, mixed devices, a grid that requires grad, both zoom and size
    _raises(ValueError, lambda: V.zoom_grids(g[0, 0], zoom=2))
    _raises(ValueError, lambda: V.zoom_grids(g[None], zoom=2))
    _raises(ValueError, lambda: V.spline_coefficients(torch.zeros((1, 4, 0, 5), device=dev)))
    _raises(ValueError, lambda: V.zoom_grids(g, size=(4, 0, 5)))
    _raises(ValueError, lambda: V.zoom_grids(g, zoom=2, order=2))
    _raises(ValueError, lambda: V.zoom_grids(g, zoom=2, size=(8, 6, 10)))
    _raises(ValueError, lambda: V.zoom_grids(g.clone().requires_grad_(True), zoom=2))
    _raises(ValueError, lambda: V.sample_grids(g, torch.zeros((1, 2, 2), device=dev)))
    _raises(ValueError, lambda: V.sample_grids(g, torch.zeros((2, 2, 3), device=dev)))
    _raises(ValueError, lambda: V.zoom_grids(g.long(), zoom=2))
    _raises(ValueError, lambda: ops.spline_prefilter(g[0]))
    _raises(ValueError, lambda: ops.spline_zoom(g, (8, 6, 10), order=2))
    _raises(ValueError, lambda: ops.spline_zoom(g.double(), (8, 6, 10)))
    _raises(ValueError, lambda: ops.spline_sample(g, p[0]))
    if dev != "cpu":
        _raises(RuntimeError, lambda: V.sample_grids(g, p.cpu()))
        _raises(RuntimeError, lambda: ops.spline_sample(g, p.cpu()))
    # from the raw entries
    lib = L.load()
    out = torch.zeros((1, 8, 6, 10), device=dev)
    v = torch.zeros((1, 2), device=dev)
    big = L.abi.core_defines("spline_core.h")["SG_SPLINE_MAX_AXIS"] + 1
    calls = [lambda: lib.sg_spline_prefilter(L.ptr(g), 1, 4, 0, 5, L.ptr(out), L.stream()),
             lambda: lib.sg_spline_prefilter(L.ptr(g), 1, 4, 3, big, L.ptr(out), L.stream()),
             lambda: lib.sg_spline_prefilter(L.ptr(g), -1, 4, 3, 5, L.ptr(out), L.stream()),
             lambda: lib.sg_spline_prefilter(L.ptr(g), 1, 4, 3, 5, None, L.stream()),
             lambda: lib.sg_spline_prefilter(L.ptr(g), 1, 4, 3, 5, L.ptr(g), L.stream()),
             lambda: lib.sg_spline_zoom(L.ptr(g), 1, 4, 3, 5, 8, 6, 10, 2, L.ptr(out), L.stream()),
             lambda: lib.sg_spline_zoom(L.ptr(g), 1, 4, 3, 5, 8, 0, 10, 3, L.ptr(out), L.stream()),
             lambda: lib.sg_spline_zoom(L.ptr(g), 1, 4, 3, 5, 8, 6, big, 3, L.ptr(out), L.stream()),
             lambda: lib.sg_spline_zoom(L.ptr(g), 1, 0, 3, 5, 8, 6, 10, 3, L.ptr(out), L.stream()),
             lambda: lib.sg_spline_zoom(None, 1, 4, 3, 5, 8, 6, 10, 3, L.ptr(out), L.stream()),
             lambda: lib.sg_spline_sample(L.ptr(g), 1, 4, 3, 0, L.ptr(p), 2, 1.0, L.ptr(v), None, L.stream()),
             lambda: lib.sg_spline_sample(L.ptr(g), 1, 4, 3, 5, L.ptr(p), -1, 1.0, L.ptr(v), None, L.stream()),
             lambda: lib.sg_spline_sample(L.ptr(g), 1, 4, 3, 5, None, 2, 1.0, L.ptr(v), None, L.stream()),
             lambda: lib.sg_spline_prefilter_form(4, 0, 5),
             lambda: lib.sg_spline_zoom_form(4, 3, 5, 8, 6, 0)]
    for call in calls:
        L.note_device(g)
        try:
            assert call() == ERR_ARG
        finally:
            L.reset_call_state()
    assert (out == 0).all() and (v == 0).all()              # refused before any launch


def check_input_forms(dev):
    """numpy arrays, float64 and float16, non-contiguous views, 3-D and 4-D: the same fp32 work."""
    x = grid((6, 5, 9))
    want = V.zoom_grids(t(x, dev), zoom=2)
    assert want.shape == (12, 10, 18) and want.dtype == torch.float32
    assert torch.equal(V.zoom_grids(t(x.astype(np.float64), dev), zoom=2), want)
    assert torch.equal(V.zoom_grids(t(x[None], dev), zoom=2)[0], want)
    assert torch.equal(V.zoom_grids(t(np.ascontiguousarray(x.transpose(2, 1, 0)), dev).permute(2, 1, 0), zoom=2), want)
    assert torch.equal(V.zoom_grids(t(x, dev), zoom=(2, 2, 2)), want) and torch.equal(V.zoom_grids(t(x, dev), size=(12, 10, 18)), want)
    assert torch.equal(V.zoom_grids(V.spline_coefficients(t(x, dev)), zoom=2, coefficients=True), want)
    assert V.zoom_grids(t(x, dev)).shape == (24, 20, 36)                                              # the default is the reference's 4
    if dev == "cpu":
        assert torch.equal(V.zoom_grids(x, zoom=2), want)
    half = t(x.astype(np.float16), dev)
    assert torch.equal(V.zoom_grids(half, zoom=2), V.zoom_grids(half.float(), zoom=2))
    assert V.max_grids_per_call((32, 32, 32), (128, 128, 128)) == 1024 and V.max_grids_per_call((4096, 4096, 4096)) == 1


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def sphere_sdf(R0=16, radius=0.5):
    """The SDF of a sphere on the R0^3 lattice that marching_cubes(spacing=2 / R0, origin=-1, pad=True) places: sample i at
    (i + 1) 2 / R0 - 1.  The sphere sits at the lattice's centre."""
    c = (np.arange(R0) + 1) * 2.0 / R0 - 1
    centre = (c[0] + c[-1]) / 2
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    return (np.sqrt((x - centre) ** 2 + (y - centre) ** 2 + (z - centre) ** 2) - radius).astype(np.float32), centre


def check_marching_cubes_upscale(dev):
    from shapegan_amd import mesh as M
    R0, up, radius = 16, 4, 0.5
    sdf, centre = sphere_sdf(R0, radius)
    g = t(sdf, dev)
    plain = M.marching_cubes(g, spacing=2.0 / R0, origin=-1.0).mesh(0)
    fine = M.marching_cubes(g, spacing=2.0 / R0, origin=-1.0, upscale=up).mesh(0)
    coarse_voxel = 2.0 / R0
    fine_voxel = coarse_voxel * (R0 - 1) / (R0 * up - 1)
    assert len(fine.vertices) > 8 * len(plain.vertices)
    assert np.abs(fine.vertices.mean(axis=0) - plain.vertices.mean(axis=0)).max() <= fine_voxel / 2
    r_fine = np.linalg.norm(fine.vertices.astype(np.float64) - centre, axis=1)
    r_plain = np.linalg.norm(plain.vertices.astype(np.float64) - centre, axis=1)
    print("radius error: plain %.4g (voxel %.4g), upscaled %.4g (voxel %.4g)" % (np.abs(r_plain - radius).max(), coarse_voxel,
                                                                                   np.abs(r_fine - radius).max(), fine_voxel))
    assert np.abs(r_fine - radius).max() <= fine_voxel and np.abs(r_plain - radius).max() <= coarse_voxel
    same = M.marching_cubes(g, spacing=2.0 / R0, origin=-1.0, upscale=None)
    base = M.marching_cubes(g, spacing=2.0 / R0, origin=-1.0)
    assert torch.equal(same.vertices, base.vertices) and torch.equal(same.faces, base.faces)


def check_render_voxels_upscale(dev):
    from shapegan_amd.rendering import MeshRenderer
    sdf, _ = sphere_sdf(16)
    grids = t(np.stack([sdf, sdf + 0.1]), dev)
    r = MeshRenderer(size=48, ssaa=1, shadow_size=64)
    base = r.render_voxels(grids, return_tensor=True)
    assert torch.equal(r.render_voxels(grids, return_tensor=True, upscale=None), base)
    up = r.render_voxels(grids, return_tensor=True, upscale=2)
    assert up.shape == base.shape == (2, 48, 48, 3) and up.dtype == torch.uint8 and not torch.equal(up, base)
    r.set_voxels(grids[0])
    a = r.get_image()
    r.set_voxels(grids[0], upscale=None)
    assert np.array_equal(r.get_image(), a)
    r.set_voxels(grids[0], upscale=2)
    b = r.get_image()
    assert b.shape == a.shape == (48, 48, 3) and np.isfinite(b.astype(np.float64)).all() and not np.array_equal(a, b)


def check_sample_from_voxels_upscale(dev, monkeypatch):
    from shapegan_amd import metrics
    monkeypatch.setattr(metrics, "device", torch.device(dev))
    sdf, _ = sphere_sdf(16)
    voxels = np.stack([sdf, sdf + 0.1, np.ones_like(sdf)])

    def run(**kw):
        torch.manual_seed(3)
        return metrics.sample_from_voxels(voxels, 64, **kw)

    base = run()
    assert np.array_equal(run(upscale=None), base)
    up = run(upscale=2)
    assert up.shape == base.shape == (3, 64, 3) and np.isfinite(up).all() and (up[2] == 0).all() and (up[0] != 0).any()
    # half_unit_sphere: the farthest point of a cloud is at 0.5; the upscaled surface is rounder, so its points keep closer to that radius
    assert abs(np.linalg.norm(up[0], axis=1).max() - 0.5) < 1e-9
