"""An independent statement of mesh topology (include/shapegan_hip.h, K12b) in numpy and plain Python: the partition by a union-find,
the numbering by lowest vertex, the statistics in float64 with math.fsum, the edge classification, the keep rules, the compaction.
Nothing here calls the package."""
import math
from collections import defaultdict

import numpy as np


def _arrays(batch):
    return (batch.vertices.detach().cpu().numpy(), batch.normals.detach().cpu().numpy(), batch.faces.detach().cpu().numpy(),
            batch.vert_offsets.cpu().numpy(), batch.tri_offsets.cpu().numpy())


def valid_triangles(faces, n):
    return ((faces >= 0) & (faces < n)).all(axis=1) if len(faces) else np.zeros(0, dtype=bool)


def label_shape(faces, n):
    """(labels [n] with -1 for unnamed vertices, number of components) of one shape: faces [F,3] local indices."""
    parent = list(range(n))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root
    named = np.zeros(n, dtype=bool)
    for tri in faces[valid_triangles(faces, n)].tolist():
        named[tri] = True
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2])):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    labels = np.full(n, -1, dtype=np.int32)
    number = {}
    for v in range(n):                      # increasing v: a component is met first at its lowest vertex
        if named[v]:
            labels[v] = number.setdefault(find(v), len(number))
    return labels, len(number)


def shape_stats(verts, faces, labels, count):
    """Per component of one shape: dict of lists vertices, triangles, edges, open_edges, area, volume."""
    n = len(verts)
    ok = valid_triangles(faces, n)
    v64 = verts.astype(np.float64)
    area_terms, vol_terms = [[] for _ in range(count)], [[] for _ in range(count)]
    area_mag, vol_mag = [[] for _ in range(count)], [[] for _ in range(count)]
    sides = [defaultdict(lambda: [0, 0]) for _ in range(count)]
    tris = [0] * count
    for tri in faces[ok].tolist():
        c = labels[tri[0]]
        tris[c] += 1
        p0, p1, p2 = v64[tri[0]], v64[tri[1]], v64[tri[2]]
        area_terms[c].append(float(np.linalg.norm(np.cross(p1 - p0, p2 - p0))) / 2)
        vol_terms[c].append(float(np.dot(p0, np.cross(p1, p2))) / 6)
        area_mag[c].append(float(np.linalg.norm(p1 - p0) * np.linalg.norm(p2 - p0)) / 2)
        vol_mag[c].append(float(np.linalg.norm(p0) * np.linalg.norm(p1) * np.linalg.norm(p2)) / 6)
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            if a != b:
                sides[c][(min(a, b), max(a, b))][0 if a < b else 1] += 1
    return {"vertices": [int((labels == c).sum()) for c in range(count)], "triangles": tris,
            "edges": [len(sides[c]) for c in range(count)],
            "open_edges": [sum(1 for fwd, bwd in sides[c].values() if not (fwd == 1 and bwd == 1)) for c in range(count)],
            "area": [math.fsum(area_terms[c]) for c in range(count)], "volume": [math.fsum(vol_terms[c]) for c in range(count)],
            "area_magnitude": [math.fsum(area_mag[c]) for c in range(count)],
            "volume_magnitude": [math.fsum(vol_mag[c]) for c in range(count)]}


def components(batch):
    """dict: vertex_component [V], comp_offsets [S+1], shape_index [C] and the per-component arrays, all numpy."""
    verts, _, faces, vo, to = _arrays(batch)
    S = len(vo) - 1
    labels, offsets, shape_index = [], [0], []
    stats = {k: [] for k in ("vertices", "triangles", "edges", "open_edges", "area", "volume", "area_magnitude", "volume_magnitude")}
    for s in range(S):
        v, f = verts[vo[s]:vo[s + 1]], faces[to[s]:to[s + 1]]
        lab, count = label_shape(f, len(v))
        labels.append(lab)
        offsets.append(offsets[-1] + count)
        shape_index += [s] * count
        for k, val in shape_stats(v, f, lab, count).items():
            stats[k] += val
    out = {"vertex_component": np.concatenate(labels) if labels else np.zeros(0, np.int32),
           "comp_offsets": np.asarray(offsets, dtype=np.int64), "shape_index": np.asarray(shape_index, dtype=np.int64)}
    for k, val in stats.items():
        out[k] = np.asarray(val, dtype=np.int32 if k in ("vertices", "triangles", "edges", "open_edges") else np.float64)
    return out


def select(ref, rule):
    """The keep mask [C] of `rule` ('largest', True, or a dict) on the components `ref` (the dict of components())."""
    if rule is True:
        rule = {"min_area_fraction": 0.01}
    if rule == "largest":
        rule = {"largest": 1}
    C, off = len(ref["area"]), ref["comp_offsets"]
    mask = np.ones(C, dtype=bool)
    for s in range(len(off) - 1):
        ids = list(range(off[s], off[s + 1]))
        total = sum(ref["area"][i] for i in ids)      # the package adds in this order too (index_add over increasing c)
        if rule.get("largest") is not None:
            best = sorted(ids, key=lambda i: (-ref["area"][i], i))[:int(rule["largest"])]
            for i in ids:
                mask[i] &= i in best
        if rule.get("min_area_fraction") is not None:
            for i in ids:
                mask[i] &= bool(ref["area"][i] >= float(rule["min_area_fraction"]) * total)
    if rule.get("min_triangles") is not None:
        mask &= ref["triangles"] >= int(rule["min_triangles"])
    if rule.get("drop_cavities"):
        mask &= ~(ref["volume"] < 0)
    return mask


def compact(batch, ref, mask):
    """(vertices, normals, faces, vert_offsets, tri_offsets) of the kept components, numpy."""
    verts, norms, faces, vo, to = _arrays(batch)
    S = len(vo) - 1
    out_v, out_n, out_f, nvo, nto = [], [], [], [0], [0]
    for s in range(S):
        v, nr, f = verts[vo[s]:vo[s + 1]], norms[vo[s]:vo[s + 1]], faces[to[s]:to[s + 1]]
        lab = ref["vertex_component"][vo[s]:vo[s + 1]]
        keep_v = np.array([l >= 0 and bool(mask[ref["comp_offsets"][s] + l]) for l in lab], dtype=bool)
        new_index = np.cumsum(keep_v) - 1
        ok = valid_triangles(f, len(v))
        keep_f = np.array([bool(ok[i]) and bool(keep_v[f[i, 0]]) for i in range(len(f))], dtype=bool)
        out_v.append(v[keep_v])
        out_n.append(nr[keep_v])
        out_f.append(new_index[f[keep_f]].reshape(-1, 3).astype(np.int64))
        nvo.append(nvo[-1] + int(keep_v.sum()))
        nto.append(nto[-1] + int(keep_f.sum()))
    return (np.concatenate(out_v).reshape(-1, 3), np.concatenate(out_n).reshape(-1, 3), np.concatenate(out_f).reshape(-1, 3),
            np.asarray(nvo, dtype=np.int64), np.asarray(nto, dtype=np.int64))


def same_partition(labels_a, labels_b):
    """True when two label arrays describe the same partition (and the same unlabelled set), whatever the numbering."""
    a, b = np.asarray(labels_a), np.asarray(labels_b)
    if a.shape != b.shape or ((a < 0) != (b < 0)).any():
        return False
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def check_against(comps, ref):
    """Asserts that a package Components equals the reference: labels, offsets and counts exactly; area and volume within
        (64 + n / 256) * 2^-53 * M,
    n the component's triangles and M the sum of the magnitudes its terms are built from (|p1 - p0| |p2 - p0| / 2 for the area,
    |p0| |p1| |p2| / 6 for the volume).  Where it comes from: both sides hold float64 sums of the same real terms; a term of the
    package differs from numpy's by a few roundings of products of that magnitude (fused against separate steps), the tile tree adds
    10 roundings, the tiles n / 256 more, fsum none; 64 covers the constant part several times over."""
    for k in ("vertex_component", "comp_offsets", "shape_index", "vertices", "triangles", "edges", "open_edges"):
        got = getattr(comps, k).cpu().numpy()
        assert got.shape == ref[k].shape and (got == ref[k]).all(), k
    eps = (64 + ref["triangles"] / 256.0) * 2.0 ** -53
    for k in ("area", "volume"):
        got = getattr(comps, k).cpu().numpy()
        assert got.shape == ref[k].shape, k
        assert (np.abs(got - ref[k]) <= eps * ref[k + "_magnitude"]).all(), (k, np.abs(got - ref[k]).max())
