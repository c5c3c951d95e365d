"""Poison-tier bodies of mesh topology (tests/poison.py): the labelling, the statistics and the compaction write every element of every
output, ragged and empty shapes included; nothing stale is read from scratch or outputs; the emit respects its capacities; two runs are
bit-identical; a small call right after a large one equals the small call alone."""
import torch

import topology_cases as K
from poison import poisoned
from shapegan_amd import lib as L
from shapegan_amd import topology as T

CASES = ("hand", "noise", "sphere", "empty")
RULE = {"largest": 2, "min_triangles": 3}


def make(dev, name):
    if name == "hand":
        return K.hand_batch(dev)[1]
    if name == "noise":
        return K.mesh_grids(K.noise_grids(3, 12, 7), dev)      # ragged: 257-odd vertices per block boundary, hundreds of components
    if name == "sphere":
        from test_mesh import sphere_grid
        return K.mesh_grids(sphere_grid(24, 0.7)[None], dev)
    return K.pack([K.hand_meshes()["nothing"], K.hand_meshes()["no_triangles"], K.hand_meshes()["nothing"]], dev)


def snapshot(batch):
    comps = T.components(batch)
    mask = T.select(comps, RULE)
    kept = T.keep_components(batch, comps, mask)
    parts = [comps.vertex_component, comps.comp_offsets, comps.shape_index, comps.vertices, comps.triangles, comps.edges, comps.open_edges,
             comps.area, comps.volume, kept.vertices, kept.normals, kept.faces, kept.vert_offsets, kept.tri_offsets]
    return [t.clone() for t in parts]


def check_outputs_and_repeat(dev, name):
    batch = make(dev, name)
    plain = snapshot(batch)
    with poisoned() as p:
        first = snapshot(batch)
        p.renew()
        second = snapshot(batch)
        p.check_canaries()
    for got in (first, second):
        for t, q in zip(got, plain):
            if t.dtype.is_floating_point:
                assert not torch.isnan(t).any(), "an output element was not written"
            assert t.shape == q.shape and torch.equal(t, q)


def emit(batch, comps, mask, cap_v, cap_t):
    """sg_topo_keep_count / _emit with output capacities of the caller's choosing -> (vertices, normals, faces, totals)."""
    dev = batch.vertices.device
    S, V, F, C = len(batch), batch.vertices.shape[0], batch.faces.shape[0], len(comps)
    lib = L.load()
    ws = torch.empty(lib.sg_topo_keep_workspace_bytes(S, V, F) // 4, dtype=torch.int32, device=dev)
    nvo, nto = torch.empty(S + 1, dtype=torch.int64, device=dev), torch.empty(S + 1, dtype=torch.int64, device=dev)
    keep = mask.to(torch.uint8).contiguous()
    out = (torch.empty((cap_v, 3), dtype=torch.float32, device=dev), torch.empty((cap_v, 3), dtype=torch.float32, device=dev),
           torch.empty((cap_t, 3), dtype=torch.int64, device=dev))
    try:
        L.check(lib.sg_topo_keep_count(L.ptr(batch.faces), L.ptr(batch.vert_offsets), L.ptr(batch.tri_offsets), S, V, F,
                                       L.ptr(comps.vertex_component), L.ptr(comps.comp_offsets), C, L.ptr(keep), L.ptr(nvo), L.ptr(nto),
                                       L.ptr(ws), ws.numel() * 4, L.stream()), "keep_count")
        L.reset_call_state()
        L.check(lib.sg_topo_keep_emit(L.ptr(batch.vertices), L.ptr(batch.normals), L.ptr(batch.faces), L.ptr(batch.vert_offsets),
                                      L.ptr(batch.tri_offsets), S, V, F, L.ptr(nvo), L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), cap_v,
                                      cap_t, L.ptr(ws), ws.numel() * 4, L.stream()), "keep_emit")
    finally:
        L.reset_call_state()
    return out + ((int(nvo[S]), int(nto[S])),)


def check_capacities(dev):
    """With room for fewer vertices and triangles than are kept, the emit writes the leading ones and nothing behind the buffers; with
    more room than needed it leaves the rest alone."""
    batch = make(dev, "noise")
    comps = T.components(batch)
    mask = T.select(comps, RULE)
    full = T.keep_components(batch, comps, mask)
    Vn, Fn = full.vertices.shape[0], full.faces.shape[0]
    assert Vn > 40 and Fn > 40
    with poisoned() as p:
        small = emit(batch, comps, mask, Vn - 17, Fn - 33)
        large = emit(batch, comps, mask, Vn + 5, Fn + 7)
        p.check_canaries()
        assert small[3] == (Vn, Fn) and large[3] == (Vn, Fn)
        assert torch.equal(small[0], full.vertices[:Vn - 17]) and torch.equal(small[1], full.normals[:Vn - 17])
        assert torch.equal(small[2], full.faces[:Fn - 33])
        assert torch.equal(large[0][:Vn], full.vertices) and torch.equal(large[2][:Fn], full.faces)
        assert torch.isnan(large[0][Vn:]).all() and torch.isnan(large[1][Vn:]).all()      # the poison is still there
        assert (large[2][Fn:] == (0 if large[2].is_cuda else -1)).all()


def check_small_after_large(dev):
    """The large call's outputs lie where the small call's will: the small call must not see them."""
    big, small = make(dev, "noise"), make(dev, "hand")
    alone = snapshot(small)
    with poisoned() as p:
        snapshot(big)
        after = snapshot(small)
        p.check_canaries()
    snapshot(big)
    again = snapshot(small)
    for a, b, c in zip(after, again, alone):
        assert torch.equal(a, c) and torch.equal(b, c)
