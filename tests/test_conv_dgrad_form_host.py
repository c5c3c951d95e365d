"""sg_conv3d_k4s2p1_dgrad_form (libshapegan_hip.so, host code, no GPU): which kernel the input-gradient entries launch for a call.
Pins the rule of the depth-walk form of the 8^3 -> 16^3 kernel (conv_dgrad_halo_dwalk_kernel, csrc/conv3d_halo.hip): dy grids of
depth 8, more than 32 input channels, an even number of 16-channel stages, and a grid (samples x h/w tiles x 2 depth halves x row
tiles x 2 parities ph) of at least 512 workgroups — from both sides of each condition."""
import pytest

from shapegan_amd import abi, ops

F = {k[len("SG_DGRAD_FORM_"):]: v for k, v in abi.DEFINES.items() if k.startswith("SG_DGRAD_FORM_")}


def test_form_values_are_the_header_s():
    assert F == {"NONE": 0, "DSKIP4": 1, "ROWS32_4": 2, "ROWS64_4": 3, "ROWS32": 4, "ROWS64": 5, "DEPTH_WALK": 6}


@pytest.mark.parametrize("batch,cin,cout,ogrid,form", [
    (128, 64, 128, (8, 8, 8), "DEPTH_WALK"),      # the WGAN critic's input gradient / generator's ConvT 128 -> 64: 512 workgroups
    (256, 64, 128, (8, 8, 8), "DEPTH_WALK"),
    (128, 64, 32, (8, 8, 8), "DEPTH_WALK"),
    (127, 64, 32, (8, 8, 8), "ROWS64"),           # 508 workgroups
    (64, 64, 128, (8, 8, 8), "ROWS64"),           # the generator update's 64 samples: 256 workgroups
    (64, 128, 64, (8, 8, 8), "DEPTH_WALK"),       # two row tiles: 512
    (63, 128, 64, (8, 8, 8), "ROWS64"),
    (64, 64, 32, (8, 16, 8), "DEPTH_WALK"),       # two h tiles: 512
    (63, 64, 32, (8, 8, 16), "ROWS64"),
    (128, 64, 48, (8, 8, 8), "ROWS64"),           # three stages
    (128, 32, 32, (8, 8, 8), "ROWS32"),           # 32 rows
    (128, 64, 32, (4, 8, 8), "ROWS64"),           # dy depth 4
    (128, 64, 32, (16, 8, 8), "ROWS64"),          # dy depth 16
    (64, 128, 256, (4, 4, 4), "DSKIP4"),
    (128, 1, 64, (16, 16, 16), "NONE"),           # a one-channel layer
    (2, 3, 5, (2, 4, 3), "NONE"),                 # the gather kernel
])
def test_which_kernel(batch, cin, cout, ogrid, form):
    assert ops.conv_dgrad_form(batch, cin, cout, ogrid) == F[form]
