"""Which weight image the dispatching 4^3 <-> 8^3 convolution entries plan (host logic of libshapegan_hip.so, no GPU): the depth-skip
forms (tests/test_gpu_conv_depth_skip.py) read images of their own, so sg_conv3d_k4s2p1_image_layout tells the chosen form.  The
forward takes the depth-skip form wherever the 4^3 kernel runs without a channel split (batch x row tiles >= 160), the input gradient
wherever it runs with 64-row workgroups (>= 256 of them); the batch size does not enter an image otherwise."""
import ctypes

from shapegan_amd import lib as L


def _layout(kind, batch, cin, cout, r=8, nbytes=1 << 28):
    dims = (ctypes.c_int * 8)(batch, cin, cin, cin, cout, r, r, r)
    return L.load().sg_conv3d_k4s2p1_image_layout(kind, dims, nbytes)


def test_forward_image_changes_with_the_channel_split_only():
    big = [_layout(0, n, 128, 256) for n in (40, 64, 128, 256)]       # 160 workgroups and more: depth-skip form
    small = [_layout(0, n, 128, 256) for n in (8, 16, 32)]            # channel split: conv_fwd_halo4_kernel
    assert all(v and v == big[0] for v in big) and all(v and v == small[0] for v in small)
    assert big[0] != small[0]


def test_input_gradient_image_changes_with_the_row_form_only():
    big = [_layout(1, n, 128, 256) for n in (64, 128, 256)]           # 64-row workgroups: depth-skip form
    small = [_layout(1, n, 128, 256) for n in (4, 16, 30)]            # 32-row workgroups: conv_dgrad_halo32_kernel<1>
    assert all(v and v == big[0] for v in big) and all(v and v == small[0] for v in small)
    assert big[0] != small[0]


def test_other_grids_keep_one_image():
    assert _layout(0, 32, 64, 128, r=16) == _layout(0, 128, 64, 128, r=16) != 0
    assert _layout(1, 8, 64, 128, r=16) == _layout(1, 128, 64, 128, r=16) != 0
