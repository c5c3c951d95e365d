"""The k4s2p1 convolution kernels on grids whose three extents differ, and the LDS-halo forward / input-gradient kernels by position
and in every form.  Every other convolution test uses a cube R x R x R, where a kernel that swaps OH and OW in a stride, a tile count,
a FastDiv, an edge-class flag or a box origin is still right; here H != W (and mostly D != H != W) in every case.  Bodies, shape lists,
patterns, references (float64 on the CPU) and tolerances: tests/conv_patterns.py.

Case -> kernel, as read off the dispatch code (conv3d.hip, halo_*_try in conv3d_halo.hip, edge_*_try in conv3d_edge.hip) and confirmed
once with a kernel trace of this file on an MI355X (DESIGN.md section 5 has the same table):

  test_tile_forms               tile_gemm_kernel<..., FwdPatchLoader / DgradPatchLoader / WgradPatchLoader>, splitk_finalize_kernel,
                                pack_dgrad_weights_kernel; the 4x4x8 / 2x4x4 / 4x8x4 outputs are refused by every 4^3 kernel
  test_fwd_halo                 debug 0: conv_fwd_halo_kernel<1, 4> (64-row tiles chosen for small grids); 16: <2, 4> (Cout > 64) else
                                <1, 4>; 48: <1, 4>; 64: as 0 without the LDS cap; 128: <1, 8> (Cout > 64) else <1, 4>
  test_fwd_halo4                conv_fwd_halo4_kernel (whole-sample box)
  test_fwd_channel_split        conv_fwd_halo4_kernel with csplit = 8 + splitk_finalize_kernel<FwdEpi>
  test_dgrad_halo               (1, 32, 16, (6, 8, 8))      conv_dgrad_halo32_kernel<0>, ppw 1, one stage per parity (odd stage count)
                                (1, 40, 48, (2, 8, 16))     conv_dgrad_halo32_kernel<0>, ppw 1, second 32-row tile has 8 rows
                                (2, 64, 32, (4, 16, 8))     conv_dgrad_halo32_kernel<0>, two row tiles, ppw 1 / 1 / 2 / 4 / 8
                                (8, 72, 32, (4, 16, 32))    conv_dgrad_halo_kernel<0> (64 rows), ppw 4 / 1 / 2 / 4 / 8, rows 64 + 8
                                (6, 64, 32, (4, 16, 32))    conv_dgrad_halo_kernel<0>, 768 workgroups: the 32 KB LDS request
                                (3, 96, 32, (4, 4, 4))      conv_dgrad_halo32_kernel<1>, odd batch, ppw 1 / 2 / 4 / 8
                                (255, 72, 32, (4, 4, 4))    conv_dgrad_halo_kernel<1> (64 rows), ppw 4 / 1 / 2 / 4 / 8, last pair = 1 sample
                                each with pack_dgrad_frag_kernel
  test_dgrad_dispatch           the 64-row rows through sg_conv3d_k4s2p1_dgrad; test_dgrad_keep_twice: sg_conv3d_k4s2p1_dgrad_keep
  test_wgrad_halo               (2, 8, 16) and (1, 8, 8) of dy: conv_wgrad_halo_kernel<2, true> (OH == 8 alone selects it);
                                (2, 16, 8): <2, false>; (2, 8, 64, (3, 8, 16)): <4, false>; each with pack_wgrad_dy_kernel
  test_one_channel              IW = 64 / 32: conv_fwd_c1_lds_kernel<1, 1, 64> / <2, 1, 32>; IW = 16: conv_fwd_c1_kernel<1, 1>;
                                weight gradient: conv_wgrad_c1_kernel<1 / 2, 0> (OW % 16 == 0), else the gather GEMM (OW = 8)
  test_one_channel_wgrad_act    conv_wgrad_c1_kernel<1 / 2, LeakyReLU / ReLU> + wgrad_c1_finalize_kernel
  test_convT_to_one_channel     (3, 64, 1, (3, 8, 32)) convT_c1_fused_kernel<true>; (50, 24, ...) convT_c1_stream_kernel;
                                (192, 5, ...) convT_c1_all_kernel; (32, 16, 1, (4, 16, 32)) tapplane_gemm_kernel<8> + col2im_c1_kernel
  test_convT_to1_pre            64 channels on 8 x 32 / 32 x 8 planes: convT_c1_stream_kernel / convT_c1_all_kernel<true, true, true, tanh>
                                (FULL); (5, 7, (2, 3, 5)): the partial-block instantiations
  test_convT                    the halo / gather kernels above through ConvTranspose3d's three epilogues and its backward
"""
import pytest

from shapegan_amd.lib import ACT_TANH

import conv_patterns as CP
import test_gpu_ops as OPS
import test_gpu_unwritten as UNW

pytestmark = pytest.mark.gpu


# ---- 1. non-cubic grids through every family ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Ci,Co,grid", CP.TILE_CASES)
def test_tile_forms(N, Ci, Co, grid):
    CP.body_conv3d(N, Ci, Co, grid)


@pytest.mark.parametrize("N,Ci,Co,ogrid", CP.WGRAD_HALO_CASES)
@pytest.mark.parametrize("pattern", CP.WGRAD_PATTERNS)
def test_wgrad_halo(N, Ci, Co, ogrid, pattern):
    CP.body_wgrad_halo(N, Ci, Co, ogrid, pattern)


@pytest.mark.parametrize("N,Ci,Co,ogrid", CP.WGRAD_HALO_CASES)
def test_wgrad_halo_writes_every_element(N, Ci, Co, ogrid):
    """tests/test_gpu_wgrad_padding.py's poison run on these grids: no element of dw is left to the zeros it started as — dw is zero
    exactly where the dense reference is (OD = 1: the taps kd = 0 and kd = 3 see padding only) — twice, bit for bit (all four shapes
    have a single K split: the kernel writes dw itself)."""
    from shapegan_amd import ops
    x, dy, ref = CP.wgrad_inputs(N, Ci, Co, ogrid, "random")
    assert bool((ref != 0).all()) == (ogrid[0] > 1)
    xg, dyg = x.cuda(), dy.cuda()

    def check(o):
        assert bool(((o[0] != 0) == (ref != 0)).all()), "an element of dw was not written"
        OPS.close(o[0], ref, what="wgrad halo under poison")
    UNW.run_form(lambda: ops.conv_wgrad_halo_raw(dyg, xg, Ci), check, what="wgrad halo %r" % ((N, Ci, Co, ogrid),))


@pytest.mark.parametrize("N,Ci,Co,grid", CP.C1_CASES)
def test_one_channel(N, Ci, Co, grid):
    CP.body_c1(N, Ci, Co, grid)


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("N,Ci,Co,grid", CP.C1_CASES[:2])
def test_one_channel_wgrad_act(N, Ci, Co, grid, act):
    CP.body_c1_wgrad_act(N, Ci, Co, grid, act)


@pytest.mark.parametrize("N,C,Co,grid", CP.CONVT_TO1_CASES)
def test_convT_to_one_channel(N, C, Co, grid):
    CP.body_convT_to1(N, C, Co, grid)


@pytest.mark.parametrize("N,C,grid", CP.CONVT_TO1_PRE_CASES)
def test_convT_to1_pre(N, C, grid):
    CP.body_convT_to1_pre(N, C, grid)


@pytest.mark.parametrize("N,Ci,Co,grid", CP.CONVT_CASES)
def test_convT(N, Ci, Co, grid):
    CP.body_convT(N, Ci, Co, grid)


# ---- 2. the halo forward and input-gradient kernels, by position and in every form ---------------------------------------------------
@pytest.mark.parametrize("pattern", CP.PATTERNS)
@pytest.mark.parametrize("N,Ci,Co,grid", CP.FWD_HALO_CASES)
def test_fwd_halo(N, Ci, Co, grid, pattern):
    CP.body_fwd_halo(N, Ci, Co, grid, pattern, CP.FWD_HALO_DEBUGS)


@pytest.mark.parametrize("pattern", CP.PATTERNS)
def test_fwd_halo4(pattern):
    CP.body_fwd_halo(*CP.FWD_HALO4_CASE, pattern)


@pytest.mark.parametrize("pattern", CP.PATTERNS)
def test_fwd_channel_split(pattern):
    CP.body_fwd_dispatch(*CP.FWD_SPLIT_CASE, pattern)


def test_fwd_tanh():
    """One shape per forward family through the tanh epilogue."""
    CP.body_fwd_halo(*CP.FWD_HALO_CASES[1], "random", CP.FWD_HALO_DEBUGS, act=ACT_TANH)
    CP.body_fwd_halo(*CP.FWD_HALO4_CASE, "random", act=ACT_TANH)
    CP.body_fwd_dispatch(*CP.FWD_SPLIT_CASE, "random", act=ACT_TANH)


@pytest.mark.parametrize("pattern", CP.PATTERNS)
@pytest.mark.parametrize("case,impls", CP.DGRAD_HALO_CASES, ids=lambda v: "-".join(str(x) for x in v).replace(" ", ""))
def test_dgrad_halo(case, impls, pattern):
    CP.body_dgrad_halo(*case, pattern, impls)


def test_dgrad_tanh():
    """One MODE 0 and one MODE 1 shape through the tanh epilogue (single and paired stores)."""
    CP.body_dgrad_halo(2, 64, 32, (4, 16, 8), "random", (1, 9), act=ACT_TANH)
    CP.body_dgrad_halo(3, 96, 32, (4, 4, 4), "random", (1, 9), act=ACT_TANH)


@pytest.mark.parametrize("pattern", ["random", "border"])
@pytest.mark.parametrize("N,Ci,Co,ogrid", CP.DGRAD_ROWS64)
def test_dgrad_dispatch(N, Ci, Co, ogrid, pattern):
    CP.body_dgrad_dispatch(N, Ci, Co, ogrid, pattern)


def test_dgrad_keep_twice(monkeypatch):
    CP.body_dgrad_keep_twice(*CP.DGRAD_ROWS64[1], monkeypatch)
