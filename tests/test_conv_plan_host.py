"""Relations between the host-only answers of the k4/s2/p1 convolution family (libshapegan_hip.so, no GPU).  Every one of these
entries reads the plan the call itself makes (csrc/conv_common.h), so what a size query returns, what sg_conv3d_k4s2p1_image_layout
and sg_conv3d_k4s2p1_wgrad_dy_image say about a workspace of that size, and what the eligibility queries refuse must agree.

Not asserted: "sg_conv3d_k4s2p1_wgrad_dy_image returns 0 below the sg_conv3d_k4s2p1_wgrad_workspace_bytes value".  That query is the
largest need of the three kernel families (the gather kernel's 16 split-K partials often dominate), while the image is gated on the
LDS-halo kernel's own, smaller need: at 128 -> 256 channels, 2 samples, 8^3 outputs the image is served one byte below the query's
value.  This has always been so; callers give the call the query's value or more."""
import ctypes

import pytest

from shapegan_amd import lib as L

BATCHES = (1, 8, 30, 48, 64, 256)
CHANNELS = ((1, 32), (1, 64), (4, 64), (24, 48), (32, 64), (36, 80), (64, 64), (64, 128), (128, 256), (256, 512))
GRIDS = ((8, 8, 8), (16, 16, 16), (32, 32, 32), (64, 64, 64), (8, 16, 16), (16, 8, 32))      # input grids; outputs are half
SHAPES = [(b, ci, co, g) for b in BATCHES for ci, co in CHANNELS for g in GRIDS]
BIG = 1 << 28


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _layout(lib, kind, b, ci, co, g, nbytes):
    dims = (ctypes.c_int * 8)(b, ci, ci, ci, co, *g)
    return lib.sg_conv3d_k4s2p1_image_layout(kind, dims, nbytes)


def _out(g):
    return tuple(d // 2 for d in g)


def test_kept_image_fits_the_size_query(lib):
    """A workspace of exactly the queried size holds the same image as a large one; one byte less than the image itself holds none.
    Image sizes as documented: forward [ceil(Cout / 128) * 128][Cin][64] floats, input gradient [8][ceil(Cin / 64) * 64][Cout][8]."""
    served = 0
    for b, ci, co, g in SHAPES:
        fwd_query = lib.sg_conv3d_k4s2p1_fwd_workspace_bytes(b, ci, co, *_out(g))
        dgrad_query = lib.sg_conv3d_k4s2p1_dgrad_workspace_bytes(co, ci)
        fwd_image = (co + 127) // 128 * 128 * ci * 64 * 4
        dgrad_image = 8 * ((ci + 63) // 64 * 64) * co * 8 * 4
        for kind, query, image in ((0, fwd_query, fwd_image), (1, dgrad_query, dgrad_image)):
            assert query >= image
            big = _layout(lib, kind, b, ci, co, g, BIG)
            assert _layout(lib, kind, b, ci, co, g, query) == big, (kind, b, ci, co, g)
            assert _layout(lib, kind, b, ci, co, g, image - 1) == 0, (kind, b, ci, co, g)
            served += big != 0
    assert served >= 100      # the sweep reaches the kernels with kept images


def test_producer_written_dy_image_has_the_documented_layout(lib):
    """[mt_total][nslice][8][64] float4 with row tiles of 32 channels; a slice is a sample of a 4^3 grid, a depth plane of an 8^3 one."""
    served = 0
    for b, ci, co, g in SHAPES:
        o = _out(g)
        query = lib.sg_conv3d_k4s2p1_wgrad_workspace_bytes(b, ci, co, *o)
        mt, ns = ctypes.c_int(-1), ctypes.c_long(-1)
        if lib.sg_conv3d_k4s2p1_wgrad_dy_image(b, ci, co, *o, query, ctypes.byref(mt), ctypes.byref(ns)) == 1:
            served += 1
            assert o in ((4, 4, 4), (8, 8, 8)) and co % 128 == 0 and ci >= 2
            assert mt.value == co // 32
            assert ns.value == (b if o == (4, 4, 4) else b * 8)
            assert mt.value * ns.value * 8 * 64 * 16 <= query
        assert lib.sg_conv3d_k4s2p1_wgrad_dy_image(b, ci, co, *o, 0, ctypes.byref(mt), ctypes.byref(ns)) == 0
    assert served >= 20


def test_eligibility_queries_refuse_what_their_gates_exclude(lib):
    """sg_conv3d_k4s2p1_wgrad_act_eligible: Cin == 1, Cout <= 64, OW % 16 == 0, LeakyReLU / ReLU.  sg_convT3d_k4s2p1_to1_pre_eligible:
    C <= 64 and planes of at most 256 positions."""
    act_served = pre_served = 0
    for b, ci, co, g in SHAPES:
        o = _out(g)
        for act in (L.ACT_NONE, L.ACT_LEAKY, L.ACT_RELU, L.ACT_TANH):
            r = lib.sg_conv3d_k4s2p1_wgrad_act_eligible(b, ci, co, *o, act)
            if ci != 1 or co > 64 or o[2] % 16 != 0 or act not in (L.ACT_LEAKY, L.ACT_RELU):
                assert r == 0, (b, ci, co, g, act)
            act_served += r
        for c in (ci, co):
            for i in (o, g):
                r = lib.sg_convT3d_k4s2p1_to1_pre_eligible(b, c, *i)
                if c > 64 or i[1] * i[2] > 256:
                    assert r == 0, (b, c, i)
                pre_served += r
    assert act_served >= 10 and pre_served >= 100
