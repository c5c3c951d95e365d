"""Mesh topology on the device of the meshes (csrc/topology.hip; CPU tensors run on the C++ twin): connected components of a packed
MeshBatch, their statistics, and the compaction that keeps a chosen set of them.

Replaces what the reference's callers took from trimesh one mesh at a time (split, body_count, is_watertight, volume, euler_number).

    comps = components(batch)                    # Components: labels, counts, area, signed volume, open edges per component
    comps.summary()                              # per shape: how many pieces, the largest one's share of the area, watertight, volume
    cleaned, comps = clean_meshes(batch, True)   # drops every piece below 1 % of its shape's area
    cleaned, comps = clean_meshes(batch, "largest")
    cleaned, comps = clean_meshes(batch, {"largest": 2, "min_triangles": 8, "drop_cavities": True})

Definitions (connectivity, numbering, open edges, the order of the sums): include/shapegan_hip.h, K12b.

Host synchronisation: components() reads the number of components back ONCE, keep_components() the two new totals ONCE, as
marching_cubes reads its totals.  The two sorts (triangles by component, half-edges by key) are torch.sort; choosing what to keep is a
handful of torch operations on the per-component arrays.
"""
import torch

from . import lib as L
from .lib import check, f32c, ptr, stream
from .mesh import MeshBatch

TILE = L.abi.core_defines("topology_core.h")["SG_TOPO_TILE"]
DEFAULT_RULE = {"min_area_fraction": 0.01}
_RULE_KEYS = ("largest", "min_area_fraction", "min_triangles", "drop_cavities")


def _ints(nbytes, device):
    """Scratch that holds indices, parents, counts and offsets: a typed integer tensor, never a byte workspace."""
    return torch.empty(max(int(nbytes) // 4, 1), dtype=torch.int32, device=device)


class Components(object):
    """The connected components of a MeshBatch of S shapes, C in all, component c of shape s at comp_offsets[s] + c:
    vertex_component [V] int32 (-1: the vertex belongs to no triangle), comp_offsets [S+1] int64, shape_index [C] int64, and per
    component vertices / triangles / edges / open_edges [C] int32, area / volume [C] float64.  All on the batch's device."""

    def __init__(self, vertex_component, comp_offsets, shape_index, vertices, triangles, edges, open_edges, area, volume):
        self.vertex_component, self.comp_offsets, self.shape_index = vertex_component, comp_offsets, shape_index
        self.vertices, self.triangles, self.edges, self.open_edges = vertices, triangles, edges, open_edges
        self.area, self.volume = area, volume
        self.kept = None          # set by clean_meshes: the mask [C] of what it kept

    def __len__(self):
        return self.area.shape[0]

    @property
    def shapes(self):
        return self.comp_offsets.shape[0] - 1

    @property
    def watertight(self):
        """[C] bool: every edge has exactly one side in each direction."""
        return (self.triangles > 0) & (self.open_edges == 0)

    @property
    def euler(self):
        """[C] int64: vertices - edges + triangles."""
        return self.vertices.long() - self.edges.long() + self.triangles.long()

    @property
    def genus(self):
        """[C] int64: (2 - euler) / 2, the number of handles of a watertight manifold component; -1 where it is not watertight."""
        g = torch.div(2 - self.euler, 2, rounding_mode="floor")
        return torch.where(self.watertight, g, torch.full_like(g, -1))

    def counts(self):
        return self.comp_offsets[1:] - self.comp_offsets[:-1]

    def shape_sum(self, values):
        """[S]: `values` [C] added per shape in increasing component number (float64: one order, the same on every run; int64)."""
        if values.dtype.is_floating_point:
            return torch.segment_reduce(values, "sum", offsets=self.comp_offsets, initial=0.0)
        out = torch.zeros(self.shapes, dtype=values.dtype, device=values.device)
        return out.index_add_(0, self.shape_index, values)

    def summary(self):
        """Per shape, tensors [S]: "components" (int64), "largest_area_fraction" (float64: the largest component's share of the
        shape's area, 0 for a shape without triangles), "watertight" (bool: it has components and all are watertight), "volume"
        (float64: the sum of the signed volumes)."""
        count = self.counts()
        total = self.shape_sum(self.area)
        largest = torch.segment_reduce(self.area, "max", offsets=self.comp_offsets, initial=0.0)
        share = torch.where(total > 0, largest / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(total))
        leaky = self.shape_sum((~self.watertight).long())
        return {"components": count, "largest_area_fraction": share, "watertight": (count > 0) & (leaky == 0),
                "volume": self.shape_sum(self.volume)}


def components(batch):
    """The connected components of every mesh of `batch` and their statistics -> Components."""
    verts, faces = f32c(batch.vertices), batch.faces.contiguous()
    vo, to = batch.vert_offsets.contiguous(), batch.tri_offsets.contiguous()
    dev = verts.device
    S, V, F = len(batch), verts.shape[0], faces.shape[0]
    lib = L.load()
    nbytes = lib.sg_topo_label_workspace_bytes(S, V)
    if nbytes == 0:
        raise RuntimeError("components: %d shapes with %d vertices exceed the int32 limits of one call" % (S, V))
    ws = _ints(nbytes, dev)
    label = torch.empty(V, dtype=torch.int32, device=dev)
    co = torch.empty(S + 1, dtype=torch.int64, device=dev)
    try:
        check(lib.sg_topo_label(ptr(faces), ptr(vo), ptr(to), S, V, F, ptr(label), ptr(co), ptr(ws), ws.numel() * 4, stream()),
              "topo_label")
    finally:
        L.reset_call_state()
    C = int(co[S])      # the one device -> host read: the number of components sizes everything below
    tri_keys = torch.empty(F, dtype=torch.int32, device=dev)
    edge_keys = torch.empty((F, 3), dtype=torch.int64, device=dev)
    try:
        check(lib.sg_topo_keys(ptr(faces), ptr(vo), ptr(to), S, V, F, ptr(label), ptr(co), C, ptr(tri_keys), ptr(edge_keys), stream()),
              "topo_keys")
    finally:
        L.reset_call_state()
    tri_sorted, tri_order = torch.sort(tri_keys, stable=True)
    edge_sorted = torch.sort(edge_keys.reshape(-1)).values
    seg = torch.searchsorted(tri_sorted, torch.arange(C + 1, dtype=torch.int32, device=dev)).to(torch.int64)
    tiles = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    tiles[1:] = torch.cumsum((seg[1:] - seg[:-1] + (TILE - 1)) // TILE, 0)
    counts = [torch.empty(C, dtype=torch.int32, device=dev) for _ in range(4)]
    area = torch.empty(C, dtype=torch.float64, device=dev)
    volume = torch.empty(C, dtype=torch.float64, device=dev)
    sums = L.workspace("topo_stats", lib.sg_topo_stats_workspace_bytes(F, C), dev)
    try:
        check(lib.sg_topo_stats(ptr(verts), ptr(faces), ptr(vo), ptr(to), S, V, F, ptr(label), ptr(co), C, ptr(tri_order),
                                ptr(seg), ptr(tiles), ptr(edge_sorted), ptr(counts[0]), ptr(counts[1]), ptr(counts[2]), ptr(counts[3]),
                                ptr(area), ptr(volume), ptr(sums), sums.numel(), stream()), "topo_stats")
    finally:
        L.reset_call_state()
    shape_index = torch.searchsorted(co, torch.arange(C, dtype=torch.int64, device=dev), right=True) - 1
    return Components(label, co, shape_index, counts[0], counts[1], counts[2], counts[3], area, volume)


def keep_components(batch, comps, mask):
    """The MeshBatch of the components of `batch` whose entry of `mask` [C] is set: vertices, normals and triangles in their original
    relative order, faces renumbered locally, the bits of vertices and normals unchanged; vertices outside every component go."""
    verts, norms, faces = f32c(batch.vertices), f32c(batch.normals), batch.faces.contiguous()
    vo, to = batch.vert_offsets.contiguous(), batch.tri_offsets.contiguous()
    dev = verts.device
    S, V, F, C = len(batch), verts.shape[0], faces.shape[0], len(comps)
    mask = torch.as_tensor(mask, device=dev)
    if mask.shape != (C,):
        raise ValueError("keep_components: expected a mask of %d components, got %s" % (C, tuple(mask.shape)))
    keep = (mask != 0).to(torch.uint8).contiguous()
    lib = L.load()
    nbytes = lib.sg_topo_keep_workspace_bytes(S, V, F)
    if nbytes == 0:
        raise RuntimeError("keep_components: %d vertices / %d triangles exceed the int32 limits of one call" % (V, F))
    ws = _ints(nbytes, dev)
    nvo = torch.empty(S + 1, dtype=torch.int64, device=dev)
    nto = torch.empty(S + 1, dtype=torch.int64, device=dev)
    label, co = comps.vertex_component, comps.comp_offsets
    try:
        check(lib.sg_topo_keep_count(ptr(faces), ptr(vo), ptr(to), S, V, F, ptr(label), ptr(co), C, ptr(keep), ptr(nvo), ptr(nto),
                                     ptr(ws), ws.numel() * 4, stream()), "topo_keep_count")
    finally:
        L.reset_call_state()
    Vn, Fn = (int(x) for x in torch.stack([nvo[S], nto[S]]).cpu())      # the one device -> host read: the totals size the outputs
    out_v = torch.empty((Vn, 3), dtype=torch.float32, device=dev)
    out_n = torch.empty((Vn, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((Fn, 3), dtype=torch.int64, device=dev)
    try:
        check(lib.sg_topo_keep_emit(ptr(verts), ptr(norms), ptr(faces), ptr(vo), ptr(to), S, V, F, ptr(nvo), ptr(out_v), ptr(out_n),
                                    ptr(out_f), Vn, Fn, ptr(ws), ws.numel() * 4, stream()), "topo_keep_emit")
    finally:
        L.reset_call_state()
    return MeshBatch(out_v, out_n, out_f, nvo, nto)


def _rule(rule):
    if rule is True:
        return dict(DEFAULT_RULE)
    if isinstance(rule, str):
        if rule != "largest":
            raise ValueError("clean: unknown rule %r ('largest', True or a dict of %s)" % (rule, ", ".join(_RULE_KEYS)))
        return {"largest": 1}
    if isinstance(rule, dict):
        unknown = sorted(set(rule) - set(_RULE_KEYS))
        if unknown:
            raise ValueError("clean: unknown keys %s (%s)" % (unknown, ", ".join(_RULE_KEYS)))
        return dict(rule)
    raise ValueError("clean: expected 'largest', True or a dict, got %r" % (rule,))


def select(comps, rule):
    """The mask [C] (bool) of the components `rule` keeps.  "largest": per shape the component of the largest area, a tie going to
    the lower number.  A dict combines, with AND: largest=k (the k largest by area, ties to the lower number), min_area_fraction=
    (area >= fraction * the shape's area), min_triangles=, drop_cavities= (drops volume < 0).  True: {"min_area_fraction": 0.01}."""
    rule = _rule(rule)
    C, dev = len(comps), comps.area.device
    mask = torch.ones(C, dtype=torch.bool, device=dev)
    if rule.get("largest") is not None:
        # stable sorts: by area, descending (equal areas keep their numbering), then by shape
        by_area = torch.sort(comps.area, descending=True, stable=True).indices
        order = by_area[torch.sort(comps.shape_index[by_area], stable=True).indices]
        rank = torch.empty(C, dtype=torch.int64, device=dev)
        rank[order] = torch.arange(C, dtype=torch.int64, device=dev) - comps.comp_offsets[comps.shape_index[order]]
        mask &= rank < int(rule["largest"])
    if rule.get("min_area_fraction") is not None:
        mask &= comps.area >= float(rule["min_area_fraction"]) * comps.shape_sum(comps.area)[comps.shape_index]
    if rule.get("min_triangles") is not None:
        mask &= comps.triangles >= int(rule["min_triangles"])
    if rule.get("drop_cavities"):
        mask &= ~(comps.volume < 0)
    return mask


def clean_meshes(batch, rule=True):
    """(the MeshBatch of the components of `batch` that `rule` keeps (select), the Components of `batch` itself with `.kept` set
    to the mask).  A shape may come out empty."""
    comps = components(batch)
    comps.kept = select(comps, rule)
    return keep_components(batch, comps, comps.kept), comps


def clean_option(text):
    """The `clean=` value of a command line's --clean: None -> False, "default" -> True, "largest" -> "largest"."""
    return {None: False, "default": True}.get(text, text)


def summary(batch):
    """The four numbers a generated set is judged by: {"mean_components", "single_component_fraction", "watertight_fraction",
    "mean_largest_area_fraction"}; the first and the last over the shapes that have triangles, the fractions over all shapes."""
    s = components(batch).summary()
    count = s["components"]
    some = count > 0
    n = max(int(some.sum()), 1)
    return {"mean_components": float(count[some].double().sum()) / n,
            "single_component_fraction": float((count == 1).double().mean()),
            "watertight_fraction": float(s["watertight"].double().mean()),
            "mean_largest_area_fraction": float(s["largest_area_fraction"][some].sum()) / n}
