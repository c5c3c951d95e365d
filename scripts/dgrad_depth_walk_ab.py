"""A/B timing of the 8^3 -> 16^3 LDS-halo input gradient at the WGAN step's shapes (GPU box), present form against depth-walk form:
    python scripts/dgrad_depth_walk_ab.py [repeats]
Conv3d 64 -> 128 input gradient / ConvT 128 -> 64 forward at 64, 128 and 256 samples, timed with HIP events exactly as the row
`conv_dgrad_halo_kernel<0>` of bench.py's conv_kernel_table (bench.event_time_ms, 20 calls, the weight-image packing launch included):
    plain      the dispatching entry ops.conv_dgrad_raw(y8, w2, None, 64) (what production runs)
    present    the forced present form (conv_dgrad_halo_raw impl 1: conv_dgrad_halo_kernel<0>)
    walk       the forced depth-walk form (impl 129: conv_dgrad_halo_dwalk_kernel); "n/a" in a tree whose library has none
One JSON line: per (batch, form) the min / median / max in us over `repeats` (default 5) measurements of one process.  To compare two
commits run it from a checkout of each, alternately, in fresh processes (the protocol of scripts/depth_skip_ab.py)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from shapegan_amd import ops  # noqa: E402

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
w2 = torch.randn(128, 64, 4, 4, 4, device="cuda") * 0.02
out = {"tree": os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "repeats": repeats, "unit": "us"}


def measure(fn):
    try:
        fn()
        torch.cuda.synchronize()
    except RuntimeError:
        return "n/a"
    us = [bench.event_time_ms(fn, 20) * 1e3 for _ in range(repeats)]
    return {"min": round(min(us), 1), "median": round(statistics.median(us), 1), "max": round(max(us), 1)}


for nb in (64, 128, 256):
    y8 = torch.randn(nb, 128, 8, 8, 8, device="cuda")
    out["dgrad_%d" % nb] = {
        "plain": measure(lambda: ops.conv_dgrad_raw(y8, w2, None, 64)),
        "present": measure(lambda: ops.conv_dgrad_halo_raw(y8, w2, None, 64, impl=1)),
        "walk": measure(lambda: ops.conv_dgrad_halo_raw(y8, w2, None, 64, impl=129)),
    }
print(json.dumps(out))
