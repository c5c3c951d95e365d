"""Inputs, references, checks and test bodies for the k4s2p1 convolution family on grids whose three extents differ
(tests/test_gpu_conv_grids.py; re-run on the twin by tests/test_cpu_twin.py and under poison by tests/test_gpu_unwritten.py and
tests/test_poison_twin.py).  Pure Python: nothing here is a test by itself.

Patterns of the driving tensor (x of a forward, dy of an input gradient; both operands of a weight gradient):
    random    dense
    border    non-zero on the outer faces only
    interior  the complement of border
    corner    non-zero at the corner positions only (all channels)
An axis of extent <= 2 has no interior position — every position of it lies on a face, `interior` would be all zeros and `border`
dense — so the faces are taken over the axes of extent >= 3 only (OD = 1 or 2 occurs here: one or two output planes).  On a cube of
extent >= 3 this is tests/test_gpu_wgrad_padding.py's mask.

References are float64 on the CPU: F.conv3d / F.conv_transpose3d(stride=2, padding=1) on .double() inputs, autograd in float64 for
gradients, cast to float32.

Checks.  Dense outputs: OPS.close at its default (RTOL = 1e-4 of the tensor's mean magnitude).  Sparse outputs (`corner`, and any
reference that is more than half zeros): the scale of atol = RTOL * scale is the mean of |ref| over the reference's non-zero
elements — the whole-tensor mean of an output that is 1 % non-zero is a hundred times smaller than the values it holds.  Without
bias and activation a sum of zero products is an exact zero in any summation order, so for the sparse patterns the set of non-zero
output elements must equal the reference's exactly.  Every check prints `[conv-grid] family | what | max |got - ref| / (scale + |ref|)`
(to be read against RTOL) before it asserts."""
import torch
import torch.nn.functional as F

import test_gpu_ops as OPS

PATTERNS = ("random", "border", "interior", "corner")


def faces(shape):
    """1 on the outer faces of a (D, H, W) grid along its axes of extent >= 3, 0 inside."""
    m = torch.ones(tuple(shape))
    inner = tuple(slice(1, -1) if e >= 3 else slice(None) for e in shape)
    if any(e >= 3 for e in shape):
        m[inner] = 0
    return m


def corners(shape):
    m = torch.zeros(tuple(shape))
    for d in (0, -1):
        for h in (0, -1):
            for w in (0, -1):
                m[d, h, w] = 1
    return m


def shaped(t, pattern):
    """t [..., D, H, W] with `pattern` applied to its last three dimensions."""
    if pattern == "random":
        return t
    grid = t.shape[-3:]
    m = {"border": faces(grid), "interior": 1 - faces(grid), "corner": corners(grid)}[pattern]
    return t * m


def ratio(got, ref, scale):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return float(((got - ref).abs() / (scale + ref.abs())).max())


def check(got, ref, family, what, sparse=False, support=False):
    """got against the float64-made reference: OPS.close at RTOL with the scale described in the module docstring; support: the set
    of non-zero elements must be the reference's."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert float(ref.abs().max()) > 0, what + ": the reference is all zeros"
    nz = ref != 0
    sparse = sparse or float(nz.float().mean()) < 0.5
    scale = float(ref[nz].abs().mean()) if sparse else float(ref.abs().mean())
    print("[conv-grid] %s | %s | %.3g" % (family, what, ratio(got, ref, scale)))
    if support:
        same = (got != 0) == nz
        assert bool(same.all()), "%s: %d element(s) are non-zero where the reference is zero or the reverse" % (what, int((~same).sum()))
    OPS.close(got, ref, atol=OPS.RTOL * scale, what=what)


def _act(t, act, slope=0.2):
    from shapegan_amd.lib import ACT_LEAKY, ACT_NONE, ACT_TANH
    return {ACT_NONE: lambda v: v, ACT_LEAKY: lambda v: F.leaky_relu(v, slope), ACT_TANH: torch.tanh}[act](t)


def _seed(*key):
    torch.manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _what(*shape):
    return "x".join(str(s) for s in shape)


# ---- 1. non-cubic grids through every family ------------------------------------------------------------------------------------------
# (N, Cin, Cout, (D, H, W)): the grid of x for Conv3d, of the input for ConvTranspose3d
TILE_CASES = [
    (2, 3, 5, (4, 8, 6)), (1, 2, 2, (2, 6, 4)), (2, 70, 130, (4, 8, 12)),
    # near-misses of the 4^3 kernels (outputs 4x4x8, 2x4x4, 4x8x4): they must not be taken for 4^3 and must still be right
    (2, 64, 32, (8, 8, 16)), (2, 64, 32, (4, 8, 8)), (2, 64, 32, (8, 16, 8)),
]
FWD_HALO_CASES = [(1, 8, 96, (2, 16, 32)), (2, 12, 40, (8, 32, 16)), (1, 24, 130, (6, 16, 16))]
FWD_HALO_DEBUGS = (0, 16, 48, 64, 128)
FWD_HALO4_CASE = (3, 16, 40, (8, 8, 8))            # the 4^3 whole-sample kernel, through impl = 1
FWD_SPLIT_CASE = (2, 128, 256, (8, 8, 8))          # its channel-split form + finalize, through the dispatching entry
# (N, Cin, Cout, (OD, OH, OW)) of dy
WGRAD_HALO_CASES = [(1, 6, 128, (2, 8, 16)), (2, 3, 96, (1, 8, 8)), (1, 6, 128, (2, 16, 8)), (2, 8, 64, (3, 8, 16))]
WGRAD_PATTERNS = ("random", "border", "interior")
C1_CASES = [(4, 1, 24, (64, 32, 64)), (4, 1, 40, (64, 64, 32)), (4, 1, 24, (128, 64, 16))]
CONVT_TO1_CASES = [(3, 64, 1, (3, 8, 32)), (50, 24, 1, (2, 16, 8)), (192, 5, 1, (2, 3, 5)), (32, 16, 1, (4, 16, 32))]
CONVT_TO1_PRE_CASES = [(3, 64, (3, 8, 32)), (2, 64, (4, 32, 8)), (5, 7, (2, 3, 5))]
CONVT_CASES = [(2, 96, 48, (2, 4, 6)), (1, 5, 3, (3, 2, 5)), (2, 64, 32, (2, 8, 16))]
# (N, Cin, Cout, (OD, OH, OW)) of dy -> the impl values of sg_conv3d_k4s2p1_dgrad_impl to run
DGRAD_HALO_CASES = [
    ((1, 32, 16, (6, 8, 8)), (1,)),
    ((1, 40, 48, (2, 8, 16)), (1, 3)),
    ((2, 64, 32, (4, 16, 8)), (1, 3, 9, 17, 33)),
    ((8, 72, 32, (4, 16, 32)), (1, 3, 9, 17, 33)),
    ((6, 64, 32, (4, 16, 32)), (1,)),
    ((3, 96, 32, (4, 4, 4)), (1, 9, 17, 33)),
    ((255, 72, 32, (4, 4, 4)), (1, 3, 9, 17, 33)),
]
DGRAD_ROWS64 = [(8, 72, 32, (4, 16, 32)), (6, 64, 32, (4, 16, 32)), (255, 72, 32, (4, 4, 4))]


def conv_reference(x, w, b, dy):
    """(y, dx, dw, db) of y = conv3d(x, w, b) with dLoss/dy = dy, through float64."""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if b is not None else None
    y = F.conv3d(xr, wr, br, stride=2, padding=1)
    y.backward(dy.double())
    return y.detach().float(), xr.grad.float(), wr.grad.float(), br.grad.float() if b is not None else None


def body_conv3d(N, Ci, Co, grid):
    """Forward, input, weight and bias gradient through ops.conv3d_k4s2p1 (the dispatching entries); on the GPU also the forced
    gather forward."""
    from oracle import c_oracle
    from shapegan_amd import ops
    from shapegan_amd.lib import ACT_NONE
    D, H, W = grid
    _seed(N, Ci, Co, D, H, W)
    x, w, b = torch.randn(N, Ci, D, H, W), torch.randn(Co, Ci, 4, 4, 4) / (Ci * 64) ** 0.5, torch.randn(Co)
    dy = torch.randn(N, Co, D // 2, H // 2, W // 2)
    y_ref, dx_ref, dw_ref, db_ref = conv_reference(x, w, b, dy)
    what = _what(N, Ci, Co, D, H, W)
    xg, wg, bg = OPS.dev(x).requires_grad_(True), OPS.dev(w).requires_grad_(True), OPS.dev(b).requires_grad_(True)
    y = ops.conv3d_k4s2p1(xg, wg, bg)
    check(y, y_ref, "tile", "fwd " + what)
    y.backward(OPS.dev(dy))
    check(xg.grad, dx_ref, "tile", "dgrad " + what)
    check(wg.grad, dw_ref, "tile", "wgrad " + what)
    check(bg.grad, db_ref, "tile", "bias grad " + what)
    if OPS.DEV == "cuda":      # (an *_impl entry has no twin)
        check(ops.conv_fwd_impl_raw(OPS.dev(x), OPS.dev(w), OPS.dev(b), ACT_NONE, 0.0, impl=0), y_ref, "tile", "gather fwd " + what)
    if N * Ci * Co * D * H * W <= 2 * 3 * 5 * 512:
        check(y, torch.from_numpy(c_oracle.conv_fwd(x.numpy(), w.numpy(), b.numpy())), "tile", "fwd vs C oracle " + what)


def fwd_inputs(N, Ci, Co, grid, pattern, act):
    """x, w, b and the float64-made reference of act(conv(x, w) + b): `random` with bias, the sparse patterns without."""
    D, H, W = grid
    _seed(N, Ci, Co, D, H, W, PATTERNS.index(pattern), act)
    x = shaped(torch.randn(N, Ci, D, H, W), pattern)
    w = torch.randn(Co, Ci, 4, 4, 4) / (Ci * 64) ** 0.5
    b = torch.randn(Co) if pattern == "random" else None
    pre = F.conv3d(x.double(), w.double(), None if b is None else b.double(), stride=2, padding=1)
    return x, w, b, _act(pre, act).float()


def _pattern_act(pattern, act):
    from shapegan_amd.lib import ACT_LEAKY, ACT_NONE
    if pattern != "random":
        return ACT_NONE
    return ACT_LEAKY if act is None else act


def body_fwd_halo(N, Ci, Co, grid, pattern, debugs=(0,), act=None):
    """conv_fwd_impl_raw(impl = 1) in every tile form `debugs` names (GPU only: an *_impl entry has no twin)."""
    from shapegan_amd import ops
    act = _pattern_act(pattern, act)
    x, w, b, ref = fwd_inputs(N, Ci, Co, grid, pattern, act)
    xg, wg, bg = OPS.dev(x), OPS.dev(w), None if b is None else OPS.dev(b)
    for debug in debugs:
        got = ops.conv_fwd_impl_raw(xg, wg, bg, act, 0.2, impl=1, debug=debug)
        check(got, ref, "fwd halo", "%s %s act %d debug %d" % (_what(N, Ci, Co, *grid), pattern, act, debug),
              sparse=pattern == "corner", support=pattern != "random")


def body_fwd_dispatch(N, Ci, Co, grid, pattern, act=None):
    """The same inputs through the dispatching forward (FWD_SPLIT_CASE: the 4^3 kernel's channel-split form + the split-K finalize)."""
    from shapegan_amd import ops
    act = _pattern_act(pattern, act)
    x, w, b, ref = fwd_inputs(N, Ci, Co, grid, pattern, act)
    got = ops.conv_fwd_raw(OPS.dev(x), OPS.dev(w), None if b is None else OPS.dev(b), act, 0.2)
    check(got, ref, "fwd dispatch", "%s %s act %d" % (_what(N, Ci, Co, *grid), pattern, act), sparse=pattern == "corner",
          support=pattern != "random")


def dgrad_inputs(N, Ci, Co, ogrid, pattern, act):
    """dy, w, b and the float64-made reference of act(conv_transpose(dy, w) + b)."""
    OD, OH, OW = ogrid
    _seed(N, Ci, Co, OD, OH, OW, PATTERNS.index(pattern), act)
    dy = shaped(torch.randn(N, Co, OD, OH, OW), pattern)
    w = torch.randn(Co, Ci, 4, 4, 4) / (Co * 8) ** 0.5
    b = torch.randn(Ci) if pattern == "random" else None
    pre = F.conv_transpose3d(dy.double(), w.double(), None if b is None else b.double(), stride=2, padding=1)
    return dy, w, b, _act(pre, act).float()


def body_dgrad_halo(N, Ci, Co, ogrid, pattern, impls=(1,), act=None):
    """conv_dgrad_halo_raw at every `impl` (1: the dispatch rule's parities per workgroup, 3: one, 1 + 4 ppw: ppw) — GPU only."""
    from shapegan_amd import ops
    act = _pattern_act(pattern, act)
    dy, w, b, ref = dgrad_inputs(N, Ci, Co, ogrid, pattern, act)
    dyg, wg, bg = OPS.dev(dy), OPS.dev(w), None if b is None else OPS.dev(b)
    for impl in impls:
        got = ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, act, 0.2, impl=impl)
        check(got, ref, "dgrad halo", "%s %s act %d impl %d" % (_what(N, Ci, Co, *ogrid), pattern, act, impl), sparse=pattern == "corner",
              support=pattern != "random")


def body_dgrad_dispatch(N, Ci, Co, ogrid, pattern):
    """The entry production calls (its own packing launch included)."""
    from shapegan_amd import ops
    act = _pattern_act(pattern, None)
    dy, w, b, ref = dgrad_inputs(N, Ci, Co, ogrid, pattern, act)
    got = ops.conv_dgrad_raw(OPS.dev(dy), OPS.dev(w), None if b is None else OPS.dev(b), Ci, act, 0.2)
    check(got, ref, "dgrad dispatch", "%s %s" % (_what(N, Ci, Co, *ogrid), pattern), sparse=pattern == "corner", support=pattern != "random")


def body_dgrad_keep_twice(N, Ci, Co, ogrid, monkeypatch):
    """conv_dgrad_raw(keep=True) twice on a weight that lives in an optimizer's flat buffer: the second call finds its packed image in
    place and skips the packing launch; both results are the reference's and equal bit for bit."""
    from shapegan_amd import ops, optim
    from shapegan_amd.lib import ACT_LEAKY
    dy, w, b, ref = dgrad_inputs(N, Ci, Co, ogrid, "random", ACT_LEAKY)
    flags = []
    real_get = ops._KEPT.get

    def spy(*a, **k):
        r = real_get(*a, **k)
        flags.append(r[1])
        return r
    monkeypatch.setattr(ops._KEPT, "get", spy)
    wp = torch.nn.Parameter(OPS.dev(w))
    opt = optim.RMSprop([wp], lr=0.05)          # (images are kept for flat-buffer parameters only)
    dyg, bg = OPS.dev(dy), OPS.dev(b)
    with torch.no_grad():
        first = ops.conv_dgrad_raw(dyg, wp, bg, Ci, ACT_LEAKY, 0.2, keep=True)
        second = ops.conv_dgrad_raw(dyg, wp, bg, Ci, ACT_LEAKY, 0.2, keep=True)
    if OPS.DEV == "cuda":                        # (the twin packs nothing: nothing to keep)
        assert flags == [False, True], flags
    check(first, ref, "dgrad dispatch", "%s keep, packing" % _what(N, Ci, Co, *ogrid))
    assert torch.equal(first, second), "the call on the kept image differs from the one that packed it"


def wgrad_inputs(N, Ci, Co, ogrid, pattern):
    """x, dy (both patterned, as in tests/test_gpu_wgrad_padding.py) and the float64-made weight gradient."""
    OD, OH, OW = ogrid
    _seed(N, Ci, Co, OD, OH, OW, PATTERNS.index(pattern))
    x = shaped(torch.randn(N, Ci, 2 * OD, 2 * OH, 2 * OW), pattern)
    dy = shaped(torch.randn(N, Co, OD, OH, OW), pattern)
    w = torch.zeros(Co, Ci, 4, 4, 4, dtype=torch.float64, requires_grad=True)
    F.conv3d(x.double(), w, None, stride=2, padding=1).backward(dy.double())
    return x, dy, w.grad.float()


def body_wgrad_halo(N, Ci, Co, ogrid, pattern):
    """conv_wgrad_halo_raw — GPU only."""
    from shapegan_amd import ops
    x, dy, ref = wgrad_inputs(N, Ci, Co, ogrid, pattern)
    got = ops.conv_wgrad_halo_raw(OPS.dev(dy), OPS.dev(x), Ci)
    check(got, ref, "wgrad halo", "%s %s" % (_what(N, Ci, Co, *ogrid), pattern))


def body_c1(N, Ci, Co, grid):
    """Conv3d(1 -> Cout <= 64) forward and weight gradient through the dispatching entries (batch * O^3 >= 65536 selects the
    one-channel kernels), bias + LeakyReLU on the forward."""
    from shapegan_amd import ops
    from shapegan_amd.lib import ACT_LEAKY
    assert Ci == 1
    D, H, W = grid
    _seed(N, Co, D, H, W)
    x = torch.rand(N, 1, D, H, W) * 2 - 1
    w, b = torch.randn(Co, 1, 4, 4, 4) * 0.2, torch.randn(Co) * 0.1
    dy = torch.randn(N, Co, D // 2, H // 2, W // 2)
    pre, _, dw_ref, _ = conv_reference(x, w, b, dy)
    what = _what(N, 1, Co, D, H, W)
    check(ops.conv_fwd_raw(OPS.dev(x), OPS.dev(w), OPS.dev(b), ACT_LEAKY, 0.2), F.leaky_relu(pre, 0.2), "one-channel", "fwd " + what)
    check(ops.conv_wgrad_raw(OPS.dev(dy), OPS.dev(x), 1), dw_ref, "one-channel", "wgrad " + what)


def body_c1_wgrad_act(N, Ci, Co, grid, act):
    """The fused activation-backward weight gradient (conv_wgrad_act_raw) for LeakyReLU (1) / ReLU (2)."""
    from shapegan_amd import ops
    from shapegan_amd import lib as L
    assert Ci == 1
    D, H, W = grid
    _seed(N, Co, D, H, W, act)
    assert L.load().sg_conv3d_k4s2p1_wgrad_act_eligible(N, 1, Co, D // 2, H // 2, W // 2, act)
    x = torch.rand(N, 1, D, H, W) * 2 - 1
    w = (torch.randn(Co, 1, 4, 4, 4) * 0.2).double().requires_grad_(True)
    b = (torch.randn(Co) * 0.1).double().requires_grad_(True)
    pre = F.conv3d(x.double(), w, b, stride=2, padding=1)
    y_ref = F.leaky_relu(pre, 0.2) if act == 1 else F.relu(pre)
    dy = torch.randn(y_ref.shape)
    dy[pre.detach().abs() < 1e-5] = 0      # a pre-activation within rounding of the kink may take either branch on the GPU
    y_ref.backward(dy.double())
    dw, db = ops.conv_wgrad_act_raw(OPS.dev(dy), OPS.dev(y_ref.detach().float()), OPS.dev(x), act, 0.2)
    what = "%s act %d" % (_what(N, 1, Co, D, H, W), act)
    check(dw, w.grad.float(), "one-channel", "dw through activation " + what)
    check(db, b.grad.float(), "one-channel", "db through activation " + what)


def body_convT_to1(N, C, Co, grid):
    """ConvTranspose3d(C -> 1) + tanh through ops.conv_transpose3d_k4s2p1 (the dispatching entry)."""
    from shapegan_amd import ops
    from shapegan_amd.lib import ACT_TANH
    assert Co == 1
    D, H, W = grid
    _seed(N, C, D, H, W)
    x, w, b = torch.randn(N, C, D, H, W), torch.randn(C, 1, 4, 4, 4) / (C * 8) ** 0.5, torch.randn(1)
    ref = torch.tanh(F.conv_transpose3d(x.double(), w.double(), b.double(), stride=2, padding=1)).float()
    with torch.no_grad():
        got = ops.conv_transpose3d_k4s2p1(OPS.dev(x), OPS.dev(w), OPS.dev(b), ACT_TANH, 0.0)
    check(got, ref, "convT C->1", _what(N, C, 1, D, H, W))


def body_convT_to1_pre(N, C, grid):
    """conv_transpose3d_to1_pre_raw (input transform scale / shift / LeakyReLU, tanh on the output): the dispatching entry against
    float64; on the GPU every kernel form — 1, 2, 5 - 8 bit-equal to each other, form 1 against float64."""
    from shapegan_amd import ops
    from shapegan_amd.lib import ACT_LEAKY, ACT_TANH
    D, H, W = grid
    _seed(N, C, D, H, W, 1)
    x, w, b = torch.randn(N, C, D, H, W), torch.randn(C, 1, 4, 4, 4) / (C * 8) ** 0.5, torch.randn(1)
    scale, shift = torch.randn(C), torch.randn(C) * 0.3
    t = F.leaky_relu(x.double() * scale.double().view(1, C, 1, 1, 1) + shift.double().view(1, C, 1, 1, 1), 0.2)
    ref = torch.tanh(F.conv_transpose3d(t, w.double(), b.double(), stride=2, padding=1)).float()
    xg, wg, bg, sg, hg = OPS.dev(x), OPS.dev(w), OPS.dev(b), OPS.dev(scale), OPS.dev(shift)
    what = _what(N, C, D, H, W)
    assert ops.convT_to1_pre_served(xg, wg)
    check(ops.conv_transpose3d_to1_pre_raw(xg, sg, hg, ACT_LEAKY, 0.2, wg, bg, ACT_TANH, 0.0), ref, "convT C->1", "to1_pre form 0 " + what)
    if OPS.DEV != "cuda":      # (kernel forms exist on the GPU only)
        return
    one = ops.conv_transpose3d_to1_pre_raw(xg, sg, hg, ACT_LEAKY, 0.2, wg, bg, ACT_TANH, 0.0, form=1)
    check(one, ref, "convT C->1", "to1_pre form 1 " + what)
    for form in (2, 5, 6, 7, 8):
        other = ops.conv_transpose3d_to1_pre_raw(xg, sg, hg, ACT_LEAKY, 0.2, wg, bg, ACT_TANH, 0.0, form=form)
        assert torch.equal(one, other), "to1_pre form %d differs from form 1 at %s" % (form, what)


def body_convT(N, Ci, Co, grid):
    """nn.ConvTranspose3d(k4, s2, p1) with the three epilogues: forward, input, weight and bias gradient (tests/test_gpu_ops.py's
    test_conv_transpose3d on a grid of three extents)."""
    from shapegan_amd import ops
    from shapegan_amd.lib import ACT_LEAKY, ACT_NONE, ACT_TANH
    D, H, W = grid
    _seed(N, Ci, Co, D, H, W, 2)
    x, w, b = torch.randn(N, Ci, D, H, W), torch.randn(Ci, Co, 4, 4, 4) / (Ci * 8) ** 0.5, torch.randn(Co)
    for act in (ACT_NONE, ACT_LEAKY, ACT_TANH):
        xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
        pre = F.conv_transpose3d(xr, wr, br, stride=2, padding=1)
        y_ref = _act(pre, act)
        dy = torch.randn(y_ref.shape)
        if act == ACT_LEAKY:
            dy[pre.detach().abs() < 1e-5] = 0      # (the kink, as in body_c1_wgrad_act)
        y_ref.backward(dy.double())
        xg, wg, bg = OPS.dev(x).requires_grad_(True), OPS.dev(w).requires_grad_(True), OPS.dev(b).requires_grad_(True)
        y = ops.conv_transpose3d_k4s2p1(xg, wg, bg, act, 0.2)
        what = "%s act %d" % (_what(N, Ci, Co, D, H, W), act)
        check(y, y_ref.detach().float(), "convT", "fwd " + what)
        y.backward(OPS.dev(dy))
        check(xg.grad, xr.grad.float(), "convT", "dgrad " + what)
        check(wg.grad, wr.grad.float(), "convT", "wgrad " + what)
        check(bg.grad, br.grad.float(), "convT", "bias grad " + what)


# One non-cubic case per family through the dispatching entries only: what the twin tier (tests/test_cpu_twin.py) and the poison tiers
# (tests/test_gpu_unwritten.py, tests/test_poison_twin.py) re-run.
DISPATCH_BODIES = [
    (body_conv3d, (2, 3, 5, (4, 8, 6))), (body_conv3d, (2, 64, 32, (8, 8, 16))),
    (body_fwd_dispatch, FWD_SPLIT_CASE + ("border",)),
    (body_dgrad_dispatch, (6, 64, 32, (4, 16, 32), "border")),
    (body_c1, (4, 1, 24, (64, 32, 64))), (body_c1_wgrad_act, (4, 1, 40, (64, 64, 32), 1)),
    (body_convT_to1, (3, 64, 1, (3, 8, 32))), (body_convT_to1, (192, 5, 1, (2, 3, 5))),
    (body_convT_to1_pre, (5, 7, (2, 3, 5))),
    (body_convT, (1, 5, 3, (3, 2, 5))),
]
# ... and one per LDS-halo family through its forced entry (GPU only)
FORCED_BODIES = [
    (body_fwd_halo, (2, 12, 40, (8, 32, 16), "border", FWD_HALO_DEBUGS)),
    (body_dgrad_halo, (8, 72, 32, (4, 16, 32), "border", (1, 3))),
    (body_wgrad_halo, (1, 6, 128, (2, 8, 16), "border")),
]
