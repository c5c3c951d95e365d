"""The depth-skip forms of the 4^3 <-> 8^3 LDS-halo kernels: conv_fwd_halo4_dskip_kernel and conv_dgrad_halo_dskip_kernel
(conv3d_halo.hip).  They do the work of conv_fwd_halo4_kernel / conv_dgrad_halo_kernel<1> on 16-column MFMA tiles (one depth plane
of one sample) and do not issue the tiles whose activation operand is the zero padding beyond the depth range.  Bodies, patterns,
references (float64 on the CPU) and tolerances are those of tests/conv_patterns.py and tests/test_gpu_ops.py, unchanged.

Case -> kernel (forced through the test-only entries; the kernel table of tests/test_gpu_conv_grids.py stays as it is: a forced call
WITHOUT the new bit still runs the kernels named there):

  forward         conv_fwd_impl_raw(impl = 1, debug = 256)       conv_fwd_halo4_dskip_kernel + pack_fwd_weights_kernel (mode 1)
                  (1, 16, 32)   the minimum: two stages, one row tile of which 32 rows exist
                  (3, 24, 96)   odd stage count; the second row tile has 32 rows
                  (2, 128, 64)  16 stages
  input gradient  conv_dgrad_halo_raw(impl = 64 + ...)           conv_dgrad_halo_dskip_kernel + pack_dgrad_frag_kernel (mode 1)
                  (1, 64, 16)   one stage per parity, the lone sample of a pair
                  (3, 72, 32)   odd batch, rows 64 + 8
                  (2, 64, 48)   three stages
                  impl 65 / 67 / 73 / 81 / 97 = the dispatch rule's parities per workgroup / 1 / 2 / 4 / 8; as in the present kernel,
                  several parities per workgroup need an even stage count (Cout / 16), so (1, 64, 16) and (2, 64, 48) run one parity
                  per workgroup at every impl and (3, 72, 32) runs 1, 1, 2, 4 and 8.
  dispatch        ops.conv_fwd_raw at 80 samples x 128 output channels (160 workgroups: no channel split) and ops.conv_dgrad_raw /
                  conv3d backward / conv_transpose3d at 64 samples x 64 channels (256 workgroups of 64 rows) take the depth-skip
                  forms: bit-equal to the forced new form.  Small batches keep conv_fwd_halo4_kernel with its channel split and
                  conv_dgrad_halo32_kernel<1>.

"Counting" inputs: x (dy) = 1 everywhere and weights (1 + tap index) * (1 + co % 3), so that every sum is a small integer, exact in
fp32 in any order: each output voxel's value is the sum over its in-range taps, border voxels differ from their neighbours, and a tap
wrongly dropped or wrongly kept is an error of at least 1 at a named position.
"""
import pytest
import torch
import torch.nn.functional as F

from shapegan_amd.lib import ACT_LEAKY, ACT_NONE

import conv_patterns as CP
import test_gpu_ops as OPS
import test_gpu_unwritten as UNW

pytestmark = pytest.mark.gpu

FWD_DSKIP = 256                      # debug bit of sg_conv3d_k4s2p1_fwd_impl
DGRAD_DSKIP = 64                     # impl bit of sg_conv3d_k4s2p1_dgrad_impl
FWD_CASES = [(1, 16, 32), (3, 24, 96), (2, 128, 64)]
DGRAD_CASES = [(1, 64, 16), (3, 72, 32), (2, 64, 48)]
DGRAD_IMPLS = tuple(DGRAD_DSKIP + i for i in (1, 3, 9, 17, 33))
G8, G4 = (8, 8, 8), (4, 4, 4)


def _first_bad(got, ref):
    bad = (got != ref).nonzero()
    return "first of %d wrong elements at (n, c, d, h, w) = %s: got %r, expected %r" % (
        bad.shape[0], tuple(int(v) for v in bad[0]), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])])) if bad.numel() else "equal"


# ---- forward 8^3 -> 4^3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", CP.PATTERNS)
@pytest.mark.parametrize("N,Ci,Co", FWD_CASES)
def test_fwd_by_position(N, Ci, Co, pattern):
    """random (bias + LeakyReLU) and the by-position patterns (no bias, no activation, exact support)."""
    CP.body_fwd_halo(N, Ci, Co, G8, pattern, (FWD_DSKIP,))


@pytest.mark.parametrize("act", [ACT_NONE, ACT_LEAKY])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,Ci,Co", FWD_CASES)
def test_fwd_bias_and_activation(N, Ci, Co, bias, act):
    from shapegan_amd import ops
    x, w, b, _ = CP.fwd_inputs(N, Ci, Co, G8, "random", act)
    b = b if bias else None
    ref = CP._act(F.conv3d(x.double(), w.double(), None if b is None else b.double(), stride=2, padding=1), act).float()
    got = ops.conv_fwd_impl_raw(OPS.dev(x), OPS.dev(w), None if b is None else OPS.dev(b), act, 0.2, impl=1, debug=FWD_DSKIP)
    CP.check(got, ref, "fwd depth-skip", "%s bias %d act %d" % (CP._what(N, Ci, Co), bias, act))


def _counting_weights(Co, Ci):
    tap = torch.arange(1, 65, dtype=torch.float32).view(1, 1, 4, 4, 4)
    return tap * (1 + torch.arange(Co) % 3).float().view(Co, 1, 1, 1, 1) * torch.ones(1, Ci, 1, 1, 1)


@pytest.mark.parametrize("N,Ci,Co", FWD_CASES)
def test_fwd_counting(N, Ci, Co):
    from shapegan_amd import ops
    x, w = torch.ones(N, Ci, *G8), _counting_weights(Co, Ci)
    ref = F.conv3d(x.double(), w.double(), None, stride=2, padding=1).float()
    assert float(ref.max()) < 2 ** 24 and len(set(ref[0, 0, :, 1, 1].tolist())) >= 3      # exact in fp32; the depth border shows
    got = ops.conv_fwd_impl_raw(OPS.dev(x), OPS.dev(w), None, ACT_NONE, 0.0, impl=1, debug=FWD_DSKIP).cpu()
    print("[conv-grid] fwd depth-skip | counting %s | %s" % (CP._what(N, Ci, Co), _first_bad(got, ref)))
    assert torch.equal(got, ref), _first_bad(got, ref)


@pytest.mark.parametrize("grid", [(8, 8, 16), (8, 16, 8), (16, 8, 8), (4, 8, 8)])
def test_fwd_refuses_other_grids(grid):
    """Outputs 4x4x8, 4x8x4, 8x4x4 and 2x4x4 are not 4^3: the forced depth-skip form refuses them (the present 4^3 kernel does too:
    tests/test_gpu_conv_grids.py)."""
    from shapegan_amd import ops
    x, w = torch.randn(2, 64, *grid).cuda(), torch.randn(32, 64, 4, 4, 4).cuda()
    with pytest.raises(RuntimeError, match="not eligible"):
        ops.conv_fwd_impl_raw(x, w, None, ACT_NONE, 0.0, impl=1, debug=FWD_DSKIP)


def test_fwd_every_element_written_and_old_against_new():
    from shapegan_amd import ops
    N, Ci, Co = FWD_CASES[1]
    x, w, b, ref = CP.fwd_inputs(N, Ci, Co, G8, "random", ACT_LEAKY)
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    UNW.run_form(lambda: ops.conv_fwd_impl_raw(xg, wg, bg, ACT_LEAKY, 0.2, impl=1, debug=FWD_DSKIP),
                 lambda o: OPS.close(o[0], ref, what="fwd depth-skip under poison"), what="fwd depth-skip")
    new = ops.conv_fwd_impl_raw(xg, wg, bg, ACT_LEAKY, 0.2, impl=1, debug=FWD_DSKIP)
    old = ops.conv_fwd_impl_raw(xg, wg, bg, ACT_LEAKY, 0.2, impl=1, debug=0)
    print("[conv-grid] fwd depth-skip | against conv_fwd_halo4_kernel | max |new - old| %.3g, bit-equal %s" % (
        float((new - old).abs().max()), bool(torch.equal(new, old))))
    OPS.close(new, old, what="fwd depth-skip against the present form")


def test_fwd_infinite_weight_on_a_depth_padding_tap():
    """w[.., kd = 0, ..] = inf: the plane od = 0 reads kd = 0 from the padding only — the depth-skip form returns the sum over the
    in-range taps there (the present form: NaN); the planes od >= 1 are +-inf or NaN in both (an infinite weight times data)."""
    from shapegan_amd import ops
    N, Ci, Co = FWD_CASES[0]
    x, w, _, _ = CP.fwd_inputs(N, Ci, Co, G8, "random", ACT_NONE)
    w0 = w.clone()
    w0[:, :, 0] = 0
    winf = w.clone()
    winf[:, :, 0] = float("inf")
    ref = F.conv3d(x.double(), w0.double(), None, stride=2, padding=1).float()
    got = ops.conv_fwd_impl_raw(x.cuda(), winf.cuda(), None, ACT_NONE, 0.0, impl=1, debug=FWD_DSKIP).cpu()
    assert bool(torch.isfinite(got[:, :, 0]).all()) and not bool(torch.isfinite(got[:, :, 1:]).any())
    CP.check(got[:, :, 0], ref[:, :, 0], "fwd depth-skip", "plane od = 0 under an infinite kd = 0 weight")


# ---- input gradient 4^3 -> 8^3 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", CP.PATTERNS)
@pytest.mark.parametrize("N,Ci,Co", DGRAD_CASES)
def test_dgrad_by_position(N, Ci, Co, pattern):
    """ConvTranspose3d forward: random (bias + LeakyReLU) and the by-position patterns, at every parities-per-workgroup value."""
    CP.body_dgrad_halo(N, Ci, Co, G4, pattern, DGRAD_IMPLS)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_LEAKY])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,Ci,Co", DGRAD_CASES)
def test_dgrad_bias_and_activation(N, Ci, Co, bias, act):
    """Without bias and activation this is the Conv3d input gradient (reference: float64 autograd of F.conv3d); with them the
    ConvTranspose3d forward (reference: F.conv_transpose3d)."""
    from shapegan_amd import ops
    dy, w, b, _ = CP.dgrad_inputs(N, Ci, Co, G4, "random", act)
    b = b if bias else None
    if b is None and act == ACT_NONE:
        ref = CP.conv_reference(torch.zeros(N, Ci, *G8), w, None, dy)[1]
    else:
        ref = CP._act(F.conv_transpose3d(dy.double(), w.double(), None if b is None else b.double(), stride=2, padding=1), act).float()
    dyg, wg, bg = OPS.dev(dy), OPS.dev(w), None if b is None else OPS.dev(b)
    for impl in DGRAD_IMPLS:
        got = ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, act, 0.2, impl=impl)
        CP.check(got, ref, "dgrad depth-skip", "%s bias %d act %d impl %d" % (CP._what(N, Ci, Co), bias, act, impl))


@pytest.mark.parametrize("N,Ci,Co", DGRAD_CASES)
def test_dgrad_counting(N, Ci, Co):
    from shapegan_amd import ops
    dy, w = torch.ones(N, Co, *G4), _counting_weights(Co, Ci)
    ref = F.conv_transpose3d(dy.double(), w.double(), None, stride=2, padding=1).float()
    assert float(ref.max()) < 2 ** 24 and len(set(ref[0, 0, :, 3, 3].tolist())) >= 4
    for impl in DGRAD_IMPLS:
        got = ops.conv_dgrad_halo_raw(OPS.dev(dy), OPS.dev(w), None, Ci, ACT_NONE, 0.0, impl=impl).cpu()
        print("[conv-grid] dgrad depth-skip | counting %s impl %d | %s" % (CP._what(N, Ci, Co), impl, _first_bad(got, ref)))
        assert torch.equal(got, ref), "impl %d: %s" % (impl, _first_bad(got, ref))


@pytest.mark.parametrize("ogrid", [(4, 4, 8), (4, 8, 4), (8, 4, 4), (2, 4, 4), (4, 16, 32)])
def test_dgrad_refuses_other_grids(ogrid):
    from shapegan_amd import ops
    dy, w = torch.randn(2, 32, *ogrid).cuda(), torch.randn(32, 64, 4, 4, 4).cuda()
    with pytest.raises(RuntimeError, match="not eligible"):
        ops.conv_dgrad_halo_raw(dy, w, None, 64, ACT_NONE, 0.0, impl=DGRAD_DSKIP + 1)


def test_dgrad_every_element_written_and_old_against_new():
    from shapegan_amd import ops
    N, Ci, Co = DGRAD_CASES[1]
    dy, w, b, ref = CP.dgrad_inputs(N, Ci, Co, G4, "random", ACT_LEAKY)
    dyg, wg, bg = dy.cuda(), w.cuda(), b.cuda()
    for impl in DGRAD_IMPLS:
        what = "dgrad depth-skip impl %d" % impl
        UNW.run_form(lambda: ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, ACT_LEAKY, 0.2, impl=impl),
                     lambda o: OPS.close(o[0], ref, what=what + " under poison"), what=what)
    # the present form at this size is the 32-row kernel; at 255 samples it is conv_dgrad_halo_kernel<1>, the A/B partner
    N = 255
    dy, w, b, ref = CP.dgrad_inputs(N, Ci, Co, G4, "random", ACT_LEAKY)
    dyg, wg, bg = dy.cuda(), w.cuda(), b.cuda()
    new = ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, ACT_LEAKY, 0.2, impl=DGRAD_DSKIP + 1)
    old = ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, ACT_LEAKY, 0.2, impl=1)
    print("[conv-grid] dgrad depth-skip | against conv_dgrad_halo_kernel<1> | max |new - old| %.3g, bit-equal %s" % (
        float((new - old).abs().max()), bool(torch.equal(new, old))))
    CP.check(new, ref, "dgrad depth-skip", "255 samples, last pair = 1 sample")
    OPS.close(new, old, what="dgrad depth-skip against the present form")


def test_dgrad_infinite_weight_on_a_depth_padding_tap():
    """Output depth 0 (parity 0, q = 0) reads kd = 1 (dy depth 0) and kd = 3 (dy depth -1: padding).  With w[.., kd = 3, ..] = inf the
    depth-skip form returns the in-range sum there; output depths 2, 4, 6 read kd = 3 on data and are not finite."""
    from shapegan_amd import ops
    N, Ci, Co = DGRAD_CASES[0]
    dy, w, _, _ = CP.dgrad_inputs(N, Ci, Co, G4, "random", ACT_NONE)
    w0 = w.clone()
    w0[:, :, 3] = 0
    winf = w.clone()
    winf[:, :, 3] = float("inf")
    ref = F.conv_transpose3d(dy.double(), w0.double(), None, stride=2, padding=1).float()
    got = ops.conv_dgrad_halo_raw(dy.cuda(), winf.cuda(), None, Ci, ACT_NONE, 0.0, impl=DGRAD_DSKIP + 1).cpu()
    assert bool(torch.isfinite(got[:, :, 0]).all()) and not bool(torch.isfinite(got[:, :, 2::2]).any())
    CP.check(got[:, :, 0], ref[:, :, 0], "dgrad depth-skip", "output depth 0 under an infinite kd = 3 weight")


# ---- dispatch --------------------------------------------------------------------------------------------------------------------------
def test_dispatch_takes_the_depth_skip_forms():
    """The plain entries are bit-equal to the forced form the dispatch rules name (module docstring), at the smallest sizes that reach
    them, and meet the float64 reference.  Conv3d backward and ConvTranspose3d forward go through the same input-gradient entry."""
    from shapegan_amd import ops
    N, Ci, Co = 80, 16, 128
    x, w, b, ref = CP.fwd_inputs(N, Ci, Co, G8, "random", ACT_LEAKY)
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    plain = ops.conv_fwd_raw(xg, wg, bg, ACT_LEAKY, 0.2)
    CP.check(plain, ref, "fwd dispatch", CP._what(N, Ci, Co))
    assert torch.equal(plain, ops.conv_fwd_impl_raw(xg, wg, bg, ACT_LEAKY, 0.2, impl=1, debug=FWD_DSKIP))

    N, Ci, Co = 64, 64, 32
    dy, w, b, ref = CP.dgrad_inputs(N, Ci, Co, G4, "random", ACT_LEAKY)
    dyg, wg, bg = dy.cuda(), w.cuda(), b.cuda()
    forced = ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, ACT_LEAKY, 0.2, impl=DGRAD_DSKIP + 1)
    plain = ops.conv_dgrad_raw(dyg, wg, bg, Ci, ACT_LEAKY, 0.2)
    CP.check(plain, ref, "dgrad dispatch", CP._what(N, Ci, Co))
    assert torch.equal(plain, forced)
    with torch.no_grad():                      # ConvTranspose3d(Co -> Ci) forward: weight [in = Co, out = Ci, 4, 4, 4]
        assert torch.equal(ops.conv_transpose3d_k4s2p1(dyg, wg, bg, ACT_LEAKY, 0.2), forced)
    xg = torch.zeros(N, Ci, *G8, device="cuda", requires_grad=True)      # Conv3d(Ci -> Co) backward
    ops.conv3d_k4s2p1(xg, wg, None).backward(dyg)
    assert torch.equal(xg.grad, ops.conv_dgrad_halo_raw(dyg, wg, None, Ci, ACT_NONE, 0.0, impl=DGRAD_DSKIP + 1))
