"""Poison-tier bodies of mesh simplification (tests/poison.py): every stage writes every element of every output and every offset, ragged
last tiles and empty shapes included; nothing stale is read from scratch or outputs; the emit respects its capacities; two runs are
bit-identical; a small call right after a large one equals the small call alone."""
import numpy as np
import torch

import simplify_cases as K
from poison import poisoned
from shapegan_amd import lib as L
from shapegan_amd import simplify as SM

# (mesh, keyword arguments): ragged runs (the icosphere's clusters hold 1 .. 2562 vertices), empty shapes first, in the middle and last,
# a batch of nothing but empty shapes, the search, both placements
CASES = {"hand": ("hand", {"cells": 2}), "hand-cell": ("hand", {"cell": 0.3, "origin": (-1.05, -1.0, -0.95)}),
         "icosphere": ("icosphere", {"cells": 6}), "icosphere-one-cluster": ("icosphere", {"cells": 1}),
         "icosphere-mean": ("icosphere", {"cells": 5, "placement": "mean"}), "mixed-target": ("mixed", {"target_triangles": [500, 5, 100, 10, 0]}),
         "empty": ("empty", {"cells": 3})}


def make(dev, name):
    if name == "empty":
        h = K.hand_meshes()
        return K.pack([h["nothing"], h["no_triangles"], h["nothing"]], dev)
    return K.built(name, dev)


def snapshot(batch, kw):
    out, info = SM.simplify_meshes(batch, **kw)
    parts = [out.vertices, out.normals, out.faces, out.vert_offsets, out.tri_offsets, info["cells"], info["cell"], info["triangles_after"]]
    return [t.clone() for t in parts]


def check_outputs_and_repeat(dev, case):
    name, kw = CASES[case]
    batch = make(dev, name)
    plain = snapshot(batch, kw)
    with poisoned() as p:
        first = snapshot(batch, kw)
        p.renew()
        second = snapshot(batch, kw)
        p.check_canaries()
    expect_nan = torch.isnan(plain[0]).any(dim=1) if name == "hand" else None      # the hand batch holds a NaN coordinate of its own
    for got in (first, second):
        for i, (t, q) in enumerate(zip(got, plain)):
            if t.dtype.is_floating_point and not (i == 0 and expect_nan is not None):
                assert not torch.isnan(t).any(), "an output element was not written"
            assert t.shape == q.shape
            if t.dtype == torch.float32:
                assert torch.equal(t.contiguous().view(torch.int32), q.contiguous().view(torch.int32))
            else:
                assert torch.equal(t, q)


def stages(batch, kw, cap_v=None, cap_t=None):
    """Every stage through the C ABI with output capacities of the caller's choosing -> (keys, vertex_cluster, cluster_offsets,
    corner records, cluster vertices, cluster normals, new offsets, out vertices, out normals, out faces, totals)."""
    p = SM._Packed(batch)
    dev, S, V, F = p.dev, p.S, p.V, p.F
    lo, hi = (t.cpu().numpy() for t in SM.bounding_boxes(batch))
    grid = SM._box_grid(lo, hi, np.full(S, kw["cells"], dtype=np.int64)).upload(dev)
    keys, sorted_keys, order, sorted_cluster, vertex_cluster, co = SM._clusters(p, grid)
    C = int(co[S])
    lib = L.load()
    corner_keys = torch.empty((F, 3), dtype=torch.int64, device=dev)
    cv, cn = torch.empty((C, 3), dtype=torch.float32, device=dev), torch.empty((C, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(max(lib.sg_simplify_faces_workspace_bytes(S, C, F) // 4, 1), dtype=torch.int32, device=dev)
    nvo, nto = torch.empty(S + 1, dtype=torch.int64, device=dev), torch.empty(S + 1, dtype=torch.int64, device=dev)
    try:
        L.check(lib.sg_simplify_corners(L.ptr(p.faces), L.ptr(p.vo), L.ptr(p.to), S, V, F, L.ptr(vertex_cluster), L.ptr(corner_keys),
                                        L.stream()), "corners")
        L.reset_call_state()
        corner_sorted = torch.sort(corner_keys.reshape(-1)).values
        L.check(lib.sg_simplify_place(L.ptr(p.verts), L.ptr(p.norms), L.ptr(p.faces), L.ptr(p.vo), L.ptr(p.to), S, V, F, L.ptr(sorted_keys),
                                      L.ptr(order), L.ptr(sorted_cluster), L.ptr(corner_sorted), C, L.ptr(grid[0]), L.ptr(grid[1]), 0,
                                      L.ptr(cv), L.ptr(cn), L.stream()), "place")
        L.reset_call_state()
        L.check(lib.sg_simplify_faces_count(L.ptr(p.faces), L.ptr(p.vo), L.ptr(p.to), S, V, F, L.ptr(vertex_cluster), L.ptr(co), C,
                                            L.ptr(nvo), L.ptr(nto), L.ptr(ws), ws.numel() * 4, L.stream()), "faces_count")
        L.reset_call_state()
        Vn, Fn = int(nvo[S]), int(nto[S])
        cap_v, cap_t = Vn if cap_v is None else Vn + cap_v, Fn if cap_t is None else Fn + cap_t
        out = (torch.empty((cap_v, 3), dtype=torch.float32, device=dev), torch.empty((cap_v, 3), dtype=torch.float32, device=dev),
               torch.empty((cap_t, 3), dtype=torch.int64, device=dev))
        L.check(lib.sg_simplify_faces_emit(L.ptr(cv), L.ptr(cn), L.ptr(p.faces), L.ptr(p.vo), L.ptr(p.to), S, V, F, L.ptr(vertex_cluster), C,
                                           L.ptr(nvo), L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), cap_v, cap_t, L.ptr(ws),
                                           ws.numel() * 4, L.stream()), "faces_emit")
    finally:
        L.reset_call_state()
    return (keys, vertex_cluster, co, corner_keys, cv, cn, nvo, nto) + out + ((Vn, Fn),)


def check_every_stage_is_written(dev):
    """The intermediate arrays too: keys, cluster numbers, corner records (every slot of every triangle), the cluster table."""
    batch = make(dev, "icosphere")
    plain = stages(batch, {"cells": 6})
    with poisoned() as p:
        got = stages(batch, {"cells": 6})
        p.check_canaries()
        for t, q in zip(got[:-1], plain[:-1]):
            if t.dtype.is_floating_point:
                assert not torch.isnan(t).any(), "an element was not written"
            assert torch.equal(t, q)


def check_capacities(dev):
    """With room for fewer vertices and triangles than are kept, the emit writes the leading ones and nothing behind the buffers; with
    more room than needed it leaves the rest alone."""
    batch = make(dev, "icosphere")
    full = stages(batch, {"cells": 6})
    Vn, Fn = full[-1]
    assert Vn > 40 and Fn > 40
    with poisoned() as p:
        small = stages(batch, {"cells": 6}, -17, -33)
        large = stages(batch, {"cells": 6}, 5, 7)
        p.check_canaries()
        assert small[-1] == (Vn, Fn) and large[-1] == (Vn, Fn)
        assert torch.equal(small[8], full[8][:Vn - 17]) and torch.equal(small[9], full[9][:Vn - 17])
        assert torch.equal(small[10], full[10][:Fn - 33])
        assert torch.equal(large[8][:Vn], full[8]) and torch.equal(large[10][:Fn], full[10])
        assert torch.isnan(large[8][Vn:]).all() and torch.isnan(large[9][Vn:]).all()      # the poison is still there
        assert (large[10][Fn:] == (0 if large[10].is_cuda else -1)).all()


def check_small_after_large(dev):
    """The large call's outputs and scratch lie where the small call's will: the small call must not see them."""
    big, small = make(dev, "icosphere"), make(dev, "hand")
    kw_big, kw_small = {"cells": 10}, {"cells": 2}
    alone = snapshot(small, kw_small)
    with poisoned() as p:
        snapshot(big, kw_big)
        after = snapshot(small, kw_small)
        p.check_canaries()
    snapshot(big, kw_big)
    again = snapshot(small, kw_small)
    for a, b, c in zip(after, again, alone):
        if a.dtype == torch.float32:
            a, b, c = (t.contiguous().view(torch.int32) for t in (a, b, c))
        assert torch.equal(a, c) and torch.equal(b, c)
