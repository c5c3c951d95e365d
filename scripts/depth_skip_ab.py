"""A/B timing of the 4^3 <-> 8^3 LDS-halo kernels at the WGAN step's shapes (GPU box), present forms against depth-skip forms:
    [SHAPEGAN_HIP_LIB=<variant .so>] python scripts/depth_skip_ab.py [repeats]
Conv3d 128 -> 256 forward (8^3 -> 4^3) at 64 and 128 samples and its input gradient / ConvT forward (4^3 -> 8^3) at 64, 128 and 256
samples, each timed with HIP events exactly as the rows `conv_fwd_halo4_kernel` and `conv_dgrad_halo_kernel<1>` of bench.py's
conv_kernel_table (bench.event_time_ms, 20 calls, the weight-image packing launch included):
    plain      the dispatching entry (what production runs; with a parent library: the present kernels)
    present    the forced present form (conv_fwd_impl_raw impl 1 / conv_dgrad_halo_raw impl 1)
    dskip      the forced depth-skip form (debug 256 / impl 65); "n/a" with a library that has none
One JSON line: per (kernel, batch, form) the min / median / max in us over `repeats` (default 5) measurements of one process.
Run it alternately with the libraries to compare, in fresh processes."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from shapegan_amd import ops  # noqa: E402

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
w3 = torch.randn(256, 128, 4, 4, 4, device="cuda") * 0.02
b3 = torch.zeros(256, device="cuda")
out = {"lib": os.environ.get("SHAPEGAN_HIP_LIB", "default"), "repeats": repeats, "unit": "us"}


def measure(fn):
    try:
        fn()
        torch.cuda.synchronize()
    except RuntimeError:
        return "n/a"
    us = [bench.event_time_ms(fn, 20) * 1e3 for _ in range(repeats)]
    return {"min": round(min(us), 1), "median": round(statistics.median(us), 1), "max": round(max(us), 1)}


try:        # a library without the depth-skip forms refuses impl 65 (and would ignore debug 256)
    ops.conv_dgrad_halo_raw(torch.randn(2, 256, 4, 4, 4, device="cuda"), w3, None, 128, impl=65)
    has_dskip = True
except RuntimeError:
    has_dskip = False
for nb in (64, 128):
    x8 = torch.randn(nb, 128, 8, 8, 8, device="cuda")
    out["fwd_%d" % nb] = {
        "plain": measure(lambda: ops.conv_fwd_raw(x8, w3, b3, 1, 0.2)),
        "present": measure(lambda: ops.conv_fwd_impl_raw(x8, w3, b3, 1, 0.2, impl=1, debug=0)),
        "dskip": measure(lambda: ops.conv_fwd_impl_raw(x8, w3, b3, 1, 0.2, impl=1, debug=256)) if has_dskip else "n/a",
    }
for nb in (64, 128, 256):
    y4 = torch.randn(nb, 256, 4, 4, 4, device="cuda")
    out["dgrad_%d" % nb] = {
        "plain": measure(lambda: ops.conv_dgrad_raw(y4, w3, None, 128)),
        "present": measure(lambda: ops.conv_dgrad_halo_raw(y4, w3, None, 128, impl=1)),
        "dskip": measure(lambda: ops.conv_dgrad_halo_raw(y4, w3, None, 128, impl=65)),
    }
print(json.dumps(out))
