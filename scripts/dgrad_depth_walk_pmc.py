"""Launch target for the counter check of the depth-walk form (GPU box): the present and the depth-walk form of the 8^3 -> 16^3 input
gradient, Conv3d 64 -> 128 at 128 samples (argv[1]: another batch size), five launches each, forced through the test-only entry:
    rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32 GRBM_GUI_ACTIVE -- python scripts/dgrad_depth_walk_pmc.py
(counters in a run of their own, no other tracing).  Per launch conv_dgrad_halo_dwalk_kernel issues exactly 15/16 of the MFMA ops of
conv_dgrad_halo_kernel<0>."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shapegan_amd import ops  # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 128
w2 = torch.randn(128, 64, 4, 4, 4, device="cuda") * 0.02
y8 = torch.randn(nb, 128, 8, 8, 8, device="cuda")
for _ in range(5):
    ops.conv_dgrad_halo_raw(y8, w2, None, 64, impl=1)
    ops.conv_dgrad_halo_raw(y8, w2, None, 64, impl=129)
torch.cuda.synchronize()
