"""An independent statement of mesh simplification by quadric vertex clustering (include/shapegan_hip.h, K12c) in numpy and plain
Python.  The cell of a vertex is float32 exactly as the contract says (a subtraction, then a product); everything else is float64 with
its own loops.  Nothing here calls the package."""
import math

import numpy as np

EPS = 1e-3
MAX_CELLS = 16384
F32 = np.float32


def arrays(batch):
    return (batch.vertices.detach().cpu().numpy(), batch.normals.detach().cpu().numpy(), batch.faces.detach().cpu().numpy(),
            batch.vert_offsets.cpu().numpy(), batch.tri_offsets.cpu().numpy())


def box(verts):
    """(lo, hi) [3] float32 of the finite coordinates, 0 on an axis without one."""
    lo, hi = np.zeros(3, F32), np.zeros(3, F32)
    for k in range(3):
        col = verts[:, k][np.isfinite(verts[:, k])] if len(verts) else verts[:0, 0]
        if len(col):
            lo[k], hi[k] = col.min(), col.max()
    return lo, hi


def box_grid(verts, cells):
    """(origin [3] f32, h f32) of `cells` cells along the largest side of the bounding box; h = 1 for a box without extent."""
    lo, hi = box(verts)
    with np.errstate(all="ignore"):
        h = F32((hi - lo).astype(F32).max()) / F32(cells)
    if not (np.isfinite(h) and h > 0):
        h = F32(1.0)
    return lo, F32(h)


def cell_indices(verts, origin, h, n):
    """[V,3] int64: clamp(floor((v - o) * inv_h), 0, n - 1) in float32, 0 for a negative or non-finite product."""
    inv_h = F32(1.0) / F32(h)
    with np.errstate(all="ignore"):
        d = (verts.astype(F32) - origin.astype(F32)).astype(F32)
        p = (d * inv_h).astype(F32)
    out = np.zeros(p.shape, dtype=np.int64)
    ok = np.isfinite(p) & (p >= 0)
    out[ok] = np.minimum(np.floor(p[ok]).astype(np.float64), n - 1).astype(np.int64)
    return out


def counting(faces, n):
    return ((faces >= 0) & (faces < n)).all(axis=1) if len(faces) else np.zeros(0, dtype=bool)


def surviving(verts, faces, origin, h, n):
    """How many counting triangles have their corners in three different cells."""
    idx = cell_indices(verts, origin, h, n)
    total = 0
    for tri in faces[counting(faces, len(verts))].tolist():
        total += len({tuple(idx[i]) for i in tri}) == 3
    return total


def cholesky_solve(M, r):
    """x with M x = r for a symmetric positive definite 3x3 M, by hand."""
    L = np.zeros((3, 3))
    for i in range(3):
        for j in range(i + 1):
            acc = M[i, j] - sum(L[i, k] * L[j, k] for k in range(j))
            if i == j:
                L[i, j] = math.sqrt(acc) if acc > 0 else float("nan")      # a NaN pivot stays one
            else:
                L[i, j] = acc / L[j, j]
    w = np.zeros(3)
    for i in range(3):
        w[i] = (r[i] - sum(L[i, k] * w[k] for k in range(i))) / L[i, i]
    x = np.zeros(3)
    for i in (2, 1, 0):
        x[i] = (w[i] - sum(L[k, i] * x[k] for k in range(i + 1, 3))) / L[i, i]
    return x


def simplify_shape(verts, normals, faces, origin, h, n, placement):
    """One shape -> dict: cells [V,3], vertex_cluster [V], clusters, positions / normals [C',3] float64 of the named clusters,
    normal_norm [C'], faces [F',3] local."""
    V = len(verts)
    idx = cell_indices(verts, origin, h, n)
    cells = sorted({tuple(t) for t in idx.tolist()})
    number = {t: i for i, t in enumerate(cells)}
    vc = np.array([number[tuple(t)] for t in idx.tolist()], dtype=np.int64).reshape(V)
    C = len(cells)
    h64, o64 = float(h), origin.astype(np.float64)
    p0 = o64 + (np.array(cells, dtype=np.float64).reshape(C, 3) + 0.5) * h64
    v64, n64 = verts.astype(np.float64), normals.astype(np.float64)
    A, b = np.zeros((C, 3, 3)), np.zeros((C, 3))
    named = np.zeros(C, dtype=bool)
    kept = []
    with np.errstate(all="ignore"):
        for tri in faces[counting(faces, V)].tolist():
            pa, pb, pc = v64[tri[0]], v64[tri[1]], v64[tri[2]]
            nv = np.cross(pb - pa, pc - pa)
            length = math.sqrt(float(nv @ nv)) if nv @ nv >= 0 else float("nan")
            cl = [int(vc[i]) for i in tri]
            if length != 0:
                for c in sorted(set(cl)):
                    A[c] += np.outer(nv, nv) / length
                    b[c] += nv * float(nv @ (pa - p0[c])) / length
            if len(set(cl)) == 3:
                named[cl] = True
                kept.append(cl)
        pos, nrm, nrm_len = np.zeros((C, 3)), np.zeros((C, 3)), np.zeros(C)
        for c in range(C):
            members = np.nonzero(vc == c)[0]
            m = np.zeros(3)
            s = np.zeros(3)
            for i in members:
                m = m + v64[i]
                s = s + n64[i]
            m = m / len(members)
            if placement == "mean":
                pos[c] = m
            else:
                d = m - p0[c]
                tr = A[c, 0, 0] + A[c, 1, 1] + A[c, 2, 2]
                y = d if tr == 0 else d + cholesky_solve(A[c] + EPS * tr * np.eye(3), b[c] - A[c] @ d)
                y = np.where(y < -h64 / 2, -h64 / 2, np.where(y > h64 / 2, h64 / 2, y))
                pos[c] = p0[c] + y
            nrm_len[c] = math.sqrt(float(s @ s)) if s @ s >= 0 else float("nan")
            nrm[c] = s / nrm_len[c] if nrm_len[c] != 0 else 0.0
    new_index = np.cumsum(named) - 1
    out_faces = new_index[np.array(kept, dtype=np.int64).reshape(-1, 3)]
    return {"cells": idx, "vertex_cluster": vc, "clusters": C, "positions": pos[named], "normals": nrm[named],
            "normal_norm": nrm_len[named], "faces": out_faces.astype(np.int64)}


def bisect_cells(verts, faces, target):
    """The cells of the search the package documents: lo = 1, hi = 16384; mid moves lo when its count is <= target, else hi."""
    lo, hi = 1, MAX_CELLS
    while hi - lo > 1:
        mid = (lo + hi) // 2
        o, h = box_grid(verts, mid)
        if surviving(verts, faces, o, h, mid) <= target:
            lo = mid
        else:
            hi = mid
    return lo


def simplify(batch, cell=None, origin=(-1.0, -1.0, -1.0), cells=None, target_triangles=None, placement="quadric"):
    """The whole batch -> dict of numpy arrays: keys [V] int64, vertex_cluster [V] (batch-wide), cluster_offsets [S+1], positions /
    normals [V',3] float64, normal_norm [V'], faces [F',3], vert_offsets / tri_offsets [S+1], cells [S], cell [S] float32, unchanged [S]."""
    verts, norms, faces, vo, to = arrays(batch)
    S = len(vo) - 1
    out = {k: [] for k in ("keys", "vertex_cluster", "positions", "normals", "normal_norm", "faces", "cells", "cell", "unchanged")}
    co, nvo, nto = [0], [0], [0]
    for s in range(S):
        v, nr, f = verts[vo[s]:vo[s + 1]], norms[vo[s]:vo[s + 1]], faces[to[s]:to[s + 1]]
        same = False
        if cell is not None:
            o, h, n = np.asarray(origin, dtype=F32), F32(cell), MAX_CELLS
        else:
            if cells is not None:
                n = int(np.broadcast_to(cells, (S,))[s])
            else:
                t = int(np.broadcast_to(target_triangles, (S,))[s])
                same = len(f) <= t
                n = 1 if same else bisect_cells(v, f, t)
            o, h = box_grid(v, n)
        r = simplify_shape(v, nr, f, o, h, n, placement)
        idx = r["cells"]
        out["keys"].append((s << 42) | (idx[:, 0] << 28) | (idx[:, 1] << 14) | idx[:, 2])
        out["vertex_cluster"].append(r["vertex_cluster"] + co[-1])
        co.append(co[-1] + r["clusters"])
        if same:      # returned unchanged: every vertex, normal and triangle as it came
            r = {"positions": v.astype(np.float64), "normals": nr.astype(np.float64), "normal_norm": np.ones(len(v)), "faces": f}
        for k in ("positions", "normals", "normal_norm", "faces"):
            out[k].append(r[k])
        nvo.append(nvo[-1] + len(r["positions"]))
        nto.append(nto[-1] + len(r["faces"]))
        out["cells"].append(0 if same else n)
        out["cell"].append(h)
        out["unchanged"].append(same)
    res = {"keys": np.concatenate(out["keys"]).astype(np.int64) if S else np.zeros(0, np.int64),
           "vertex_cluster": np.concatenate(out["vertex_cluster"]), "cluster_offsets": np.asarray(co, dtype=np.int64),
           "positions": np.concatenate(out["positions"]).reshape(-1, 3), "normals": np.concatenate(out["normals"]).reshape(-1, 3),
           "normal_norm": np.concatenate(out["normal_norm"]), "faces": np.concatenate(out["faces"]).reshape(-1, 3).astype(np.int64),
           "vert_offsets": np.asarray(nvo, dtype=np.int64), "tri_offsets": np.asarray(nto, dtype=np.int64),
           "cells": np.asarray(out["cells"], dtype=np.int64), "cell": np.asarray(out["cell"], dtype=F32),
           "unchanged": np.asarray(out["unchanged"], dtype=bool)}
    return res


def volume(positions, faces):
    """The signed volume of one closed mesh, float64."""
    p = positions[faces]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6)


ULP = 2.0 ** -23


def check_against(got, ref, left_out=0.01):
    """Asserts that a package result (MeshBatch) equals the reference: offsets and faces exactly; positions and normals within one
    float32 step at the coordinate's magnitude, |got - ref64| <= 2^-23 max(1, |ref64|) (the package's double result differs from the
    reference's by the order of its sums only, far below half a step; the rounding to float32 can then differ by one step; the solve's
    condition is at most 3 / eps); a NaN where the reference has one.  Normals are compared where the reference's summed normal has
    norm >= 1e-6, and at most `left_out` (1 %) of the vertices may be left out that way (the hand-built meshes, whose point is a sum
    that cancels, raise it); where that norm is exactly zero the package's normal must be exactly zero.  Returns the worst error /
    tolerance of (positions, normals)."""
    assert np.array_equal(got.vert_offsets.cpu().numpy(), ref["vert_offsets"]), "vert_offsets"
    assert np.array_equal(got.tri_offsets.cpu().numpy(), ref["tri_offsets"]), "tri_offsets"
    assert np.array_equal(got.faces.cpu().numpy().reshape(-1, 3), ref["faces"]), "faces"
    worst = []
    for name, g, r, use in (("vertices", got.vertices, ref["positions"], None), ("normals", got.normals, ref["normals"], ref["normal_norm"])):
        g = g.cpu().numpy().astype(np.float64).reshape(-1, 3)
        assert g.shape == r.shape, name
        rows = np.ones(len(r), dtype=bool) if use is None else ~(use < 1e-6)
        if use is not None:
            assert (~rows).sum() <= left_out * max(len(r), 1), "too many normals left out"
            assert (g[use == 0] == 0).all(), "a zero sum of normals gives zeros"
        g, r = g[rows], r[rows]
        assert np.array_equal(np.isnan(g), np.isnan(r)), name + ": NaN pattern"
        fin = ~np.isnan(r)
        ratio = np.abs(g[fin] - r[fin]) / (ULP * np.maximum(1.0, np.abs(r[fin])))
        worst.append(float(ratio.max()) if ratio.size else 0.0)
        assert worst[-1] <= 1.0, (name, worst[-1])
    return tuple(worst)
