"""Launch target for the counter check of the depth-skip forms (GPU box): the present and the depth-skip form of the 8^3 -> 4^3 forward
and of the 4^3 -> 8^3 input gradient, Conv3d 128 -> 256 at 128 samples, five launches each, forced through the test-only entries:
    rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32 GRBM_GUI_ACTIVE -- python scripts/depth_skip_pmc.py
(counters in a run of their own, no other tracing).  Per launch the depth-skip forms issue 7/8 of the present forms' MFMA ops."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shapegan_amd import ops  # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 128
w3 = torch.randn(256, 128, 4, 4, 4, device="cuda") * 0.02
b3 = torch.zeros(256, device="cuda")
x8 = torch.randn(nb, 128, 8, 8, 8, device="cuda")
y4 = torch.randn(nb, 256, 4, 4, 4, device="cuda")
for _ in range(5):
    ops.conv_fwd_impl_raw(x8, w3, b3, 1, 0.2, impl=1, debug=0)
    ops.conv_fwd_impl_raw(x8, w3, b3, 1, 0.2, impl=1, debug=256)
    ops.conv_dgrad_halo_raw(y4, w3, None, 128, impl=1)
    ops.conv_dgrad_halo_raw(y4, w3, None, 128, impl=65)
torch.cuda.synchronize()
