"""Mesh simplification on the GPU against the meshing it follows, from seeded inputs only; prints one JSON line.

    python scripts/simplify_bench.py [--iters N] [--out profiles/simplify_mi355x.json]

Cases (those of scripts/topology_bench.py): 100 x 64^3 and 8 x 128^3 grids of the SDFNet with the chairs weights of tests/golden at
seeded standard-normal codes (a seeded random network when the file is missing).  Per case, in the same run: marching_cubes of the
batch (the yardstick); simplify_meshes at cells 16 / 32 / 64 and at one target_triangles, with the part of each call spent in the two
torch sorts (device events around every torch.sort inside the call) against the rest (the project's kernels, the allocations and the
host reads between them); the ratio to the meshing time; and two host baselines at cells 32: the numpy reference of the tests on the
FIRST shape alone (it is plain Python loops) and the C++ twin on the whole batch.  Device-event times around whole calls: the host
reads between their launches are inside.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from shapegan_amd import simplify as SM  # noqa: E402
from shapegan_amd.mesh import MeshBatch, marching_cubes  # noqa: E402
from shapegan_amd.model.sdf_net import SDFNet  # noqa: E402

TARGET = 2000


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        r = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, r


def sort_time(fn, iters):
    """Milliseconds per call of `fn` spent inside torch.sort, by device events around every sort."""
    real, marks = torch.sort, []

    def sort(*args, **kwargs):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = real(*args, **kwargs)
        e.record()
        marks.append((s, e))
        return out
    torch.sort = sort
    try:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    finally:
        torch.sort = real
    return sum(s.elapsed_time(e) for s, e in marks) / iters


def shape_of(batch, s):
    vo, to = batch.vert_offsets.cpu().numpy(), batch.tri_offsets.cpu().numpy()
    return MeshBatch(batch.vertices[vo[s]:vo[s + 1]].cpu(), batch.normals[vo[s]:vo[s + 1]].cpu(), batch.faces[to[s]:to[s + 1]].cpu(),
                     torch.tensor([0, vo[s + 1] - vo[s]]), torch.tensor([0, to[s + 1] - to[s]]))


def case(name, grids, iters):
    R = grids.shape[-1]
    mc_ms, batch = timed(lambda: marching_cubes(grids, level=0.0, spacing=2.0 / R, origin=-1, pad=True, pad_value=1.0), iters)
    runs = []
    for kw in ({"cells": 16}, {"cells": 32}, {"cells": 64}, {"target_triangles": TARGET}):
        ms, (out, info) = timed(lambda: SM.simplify_meshes(batch, **kw), iters)
        sorts = sort_time(lambda: SM.simplify_meshes(batch, **kw), iters)
        runs.append({"arguments": kw, "triangles_after": out.faces.shape[0], "simplify_ms": round(ms, 3), "torch_sorts_ms": round(sorts, 3),
                     "kernels_and_host_ms": round(ms - sorts, 3), "simplify_over_marching_cubes": round(ms / mc_ms, 3)})
    host = MeshBatch(batch.vertices.cpu(), batch.normals.cpu(), batch.faces.cpu(), batch.vert_offsets.cpu(), batch.tri_offsets.cpu())
    t0 = time.perf_counter()
    SM.simplify_meshes(host, cells=32)
    twin_ms = (time.perf_counter() - t0) * 1e3
    import simplify_reference
    first = shape_of(batch, 0)
    t0 = time.perf_counter()
    simplify_reference.simplify(first, cells=32)
    ref_ms = (time.perf_counter() - t0) * 1e3
    return {"case": name, "shapes": grids.shape[0], "resolution": R, "vertices": batch.vertices.shape[0], "triangles": batch.faces.shape[0],
            "marching_cubes_ms": round(mc_ms, 3), "runs": runs, "twin_cells32_ms": round(twin_ms, 3),
            "numpy_reference_first_shape_cells32_ms": round(ref_ms, 3), "first_shape_triangles": first.faces.shape[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "simplify_bench needs a GPU"
    torch.manual_seed(0)
    net = SDFNet()
    weights = os.path.join(ROOT, "tests", "golden", "sdfnet_chairs_weights.npz")
    if os.path.exists(weights):
        import numpy as np
        from shapegan_amd import lib as L
        z = np.load(weights)
        net.load_state_dict({k: torch.from_numpy(z[k]) for k in z.files})
        L.bump_param_epoch()
    net.eval()
    cases = []
    with torch.no_grad():
        for S, R in ((100, 64), (8, 128)):
            z = torch.randn(S, 128, generator=torch.Generator().manual_seed(R)).cuda()
            cases.append(case("sdfnet", net.voxel_grids(z, R, sphere_only=True, level=0.0), args.iters))
    result = {"metric": "simplify", "device": torch.cuda.get_device_name(0), "iters": args.iters, "trained_weights": os.path.exists(weights),
              "target_triangles": TARGET, "cases": cases,
              "max_simplify_over_marching_cubes": max(r["simplify_over_marching_cubes"] for c in cases for r in c["runs"])}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
