"""Mesh topology on the GPU against the meshing it follows, from seeded inputs only; prints one JSON line.

    python scripts/topology_bench.py [--iters N] [--out profiles/topology_mi355x.json]

Cases: 100 x 64^3 and 8 x 128^3 grids of the SDFNet with the chairs weights of tests/golden at seeded standard-normal codes (shapes
with floaters; a seeded random network when the file is missing), and 16 x 64^3 uniform-noise grids, the many-component extreme.
Per case, in the same run: marching_cubes of the batch (the yardstick), components (labelling + the two sorts + statistics), clean_meshes with the default rule (components + selection + compaction), their
ratio to the meshing time, and a host baseline of the labelling alone on the same mesh: scipy.sparse.csgraph.connected_components
when scipy imports, the C++ twin otherwise.  Device-event times around whole calls: the host reads between their launches are inside.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shapegan_amd import topology as T  # noqa: E402
from shapegan_amd.mesh import MeshBatch, marching_cubes  # noqa: E402
from shapegan_amd.model.sdf_net import SDFNet  # noqa: E402


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


def host_baseline(batch):
    """(name, seconds) of labelling the same mesh on the host."""
    host = MeshBatch(batch.vertices.cpu(), batch.normals.cpu(), batch.faces.cpu(), batch.vert_offsets.cpu(), batch.tri_offsets.cpu())
    try:
        import numpy as np
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        t0 = time.perf_counter()
        T.components(host)
        return "twin (labelling, sorts and statistics)", time.perf_counter() - t0
    vo, to = host.vert_offsets.numpy(), host.tri_offsets.numpy()
    faces = host.faces.numpy() + np.repeat(vo[:-1], to[1:] - to[:-1])[:, None]
    t0 = time.perf_counter()
    V = host.vertices.shape[0]
    rows, cols = np.concatenate([faces[:, 0], faces[:, 1]]), np.concatenate([faces[:, 1], faces[:, 2]])
    connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V)), directed=False)
    return "scipy.sparse.csgraph.connected_components (labelling only)", time.perf_counter() - t0


def case(name, grids, level, iters):
    R = grids.shape[-1]
    mc_ms, batch = timed(lambda: marching_cubes(grids, level=level, spacing=2.0 / R, origin=-1, pad=True, pad_value=1.0), iters)
    comp_ms, comps = timed(lambda: T.components(batch), iters)
    clean_ms, (cleaned, _) = timed(lambda: T.clean_meshes(batch, True), iters)
    base, base_s = host_baseline(batch)
    s = comps.summary()
    return {"case": name, "shapes": grids.shape[0], "resolution": R, "vertices": batch.vertices.shape[0], "triangles": batch.faces.shape[0],
            "components": len(comps), "single_component_shapes": int((s["components"] == 1).sum()),
            "triangles_after_clean": cleaned.faces.shape[0],
            "marching_cubes_ms": round(mc_ms, 3), "components_ms": round(comp_ms, 3), "clean_meshes_ms": round(clean_ms, 3),
            "clean_over_marching_cubes": round(clean_ms / mc_ms, 3), "host_baseline": base, "host_baseline_ms": round(base_s * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "topology_bench needs a GPU"
    torch.manual_seed(0)
    net = SDFNet()
    weights = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "sdfnet_chairs_weights.npz")
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
            cases.append(case("sdfnet", net.voxel_grids(z, R, sphere_only=True, level=0.0), 0.0, args.iters))
    noise = torch.rand((16, 64, 64, 64), generator=torch.Generator(device="cuda").manual_seed(7), device="cuda") * 2 - 1
    cases.append(case("noise", noise, 0.0, args.iters))
    result = {"metric": "topology", "device": torch.cuda.get_device_name(0), "iters": args.iters, "trained_weights": os.path.exists(weights),
              "cases": cases,
              "max_clean_over_marching_cubes": max(c["clean_over_marching_cubes"] for c in cases)}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
