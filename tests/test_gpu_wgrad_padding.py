"""The LDS-halo weight-gradient kernels that skip the all-padding tap rows (conv_wgrad_halo_kernel<2, true> on grids with OH == 8,
conv_wgrad_halo4_kernel on 4^3 grids) against the float64 CPU weight gradient of F.conv3d(x, w, stride=2, padding=1), with the forms
they leave alone (the generic 128-row form at OH = 16, the 64-row form) beside them.

Three input patterns per shape.  `border`: x is non-zero only on its six outer faces and dy only at the output positions on the grid's
outer faces, so the result consists of the taps next to the dropped ones alone — an off-by-one in the skip predicate or in the
(channel, tap) -> column map cannot hide under the bulk of the sum.  `interior` is its complement, `random` is dense.

Comparison and tolerance are those of tests/test_gpu_ops.py::test_conv_wgrad_halo_kernel (OPS.close at its default RTOL)."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_ops as OPS
import test_gpu_unwritten as UNW

pytestmark = pytest.mark.gpu

SHAPES = [
    # N, Cin, Cout, O
    (2, 6, 128, 8), (1, 3, 96, 8), (3, 2, 160, 8),      # static skip, 8x8-plane stages (odd Cin, partial row tiles)
    (1, 6, 128, 16),                                    # the generic form (a tile has one padded edge at most, by position)
    (2, 8, 64, 8),                                      # the 64-row form
    (4, 6, 128, 4), (5, 3, 96, 4), (8, 2, 256, 4),      # static skip, whole-sample stages (the last: more than one K split)
]
PATTERNS = ["random", "border", "interior"]


def _faces(t):
    """1 on the six outer faces of the last three dimensions, 0 inside."""
    m = torch.ones(t.shape[-3:])
    m[1:-1, 1:-1, 1:-1] = 0
    return m


def _inputs(N, Ci, Co, O, pattern):
    torch.manual_seed(1000 * PATTERNS.index(pattern) + N + Ci + Co + O)
    x, dy = torch.randn(N, Ci, 2 * O, 2 * O, 2 * O), torch.randn(N, Co, O, O, O)
    if pattern == "border":
        x, dy = x * _faces(x), dy * _faces(dy)
    elif pattern == "interior":
        x, dy = x * (1 - _faces(x)), dy * (1 - _faces(dy))
    return x, dy


def _reference(x, dy, Ci, Co):
    w = torch.zeros(Co, Ci, 4, 4, 4, dtype=torch.float64, requires_grad=True)
    F.conv3d(x.double(), w, None, stride=2, padding=1).backward(dy.double())
    return w.grad.float()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N,Ci,Co,O", SHAPES)
def test_wgrad_halo_padding_patterns(N, Ci, Co, O, pattern):
    from shapegan_amd import ops
    x, dy = _inputs(N, Ci, Co, O, pattern)
    ref = _reference(x, dy, Ci, Co)
    assert float(ref.abs().max()) > 0
    got = ops.conv_wgrad_halo_raw(OPS.dev(dy), OPS.dev(x), Ci)
    OPS.close(got, ref, what="wgrad halo, %s pattern" % pattern)


@pytest.mark.parametrize("N,Ci,Co,O", SHAPES)
def test_wgrad_halo_writes_every_element(N, Ci, Co, O):
    """Under poison (the partial-sum workspace starts as NaN, dw as zeros) and twice on the same inputs: no element of dw is left
    unwritten by the epilogue's column map — a NaN or a zero where the dense reference has a value — and both runs agree bit for bit."""
    from shapegan_amd import ops
    x, dy = _inputs(N, Ci, Co, O, "random")
    ref = _reference(x, dy, Ci, Co)
    assert bool((ref != 0).all())
    xg, dyg = x.cuda(), dy.cuda()

    def check(o):
        assert bool((o[0] != 0).all()), "an element of dw was not written"
        OPS.close(o[0], ref, what="wgrad halo under poison")
    UNW.run_form(lambda: ops.conv_wgrad_halo_raw(dyg, xg, Ci), check, what="wgrad halo (%d, %d, %d, %d)" % (N, Ci, Co, O))
