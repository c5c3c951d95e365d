"""Mesh.export (.obj, .stl, .ply) parses back to the same mesh with minimal readers written here; apply_transform and
apply_translation are the plain numpy formulas (trimesh's semantics: normals rotated and renormalised, winding reversed by a mirror)."""
import struct

import numpy as np
import pytest

from shapegan_amd.mesh import Mesh


def small_mesh(normals=True):
    """an octahedron with irrational coordinates (nothing a text format could round kindly)"""
    rng = np.random.RandomState(3)
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64) * np.pi / 3 + rng.randn(6, 3) * 0.01
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    return Mesh(v, f, n if normals else None)


def read_obj(path):
    v, n, f = [], [], []
    for line in open(path):
        t = line.split()
        if t[0] == "v":
            v.append([float(x) for x in t[1:]])
        elif t[0] == "vn":
            n.append([float(x) for x in t[1:]])
        elif t[0] == "f":
            f.append([int(x.split("/")[0]) - 1 for x in t[1:]])
            assert all(x.split("/")[-1] == x.split("/")[0] for x in t[1:])
    return np.array(v, dtype=np.float32), np.array(f), np.array(n, dtype=np.float32)


def read_stl(path):
    raw = open(path, "rb").read()
    count = struct.unpack("<I", raw[80:84])[0]
    assert len(raw) == 84 + 50 * count
    rec = np.frombuffer(raw[84:], dtype=[("normal", "<f4", 3), ("corners", "<f4", (3, 3)), ("attr", "<u2")])
    return rec["normal"], rec["corners"]


def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    props = [l.split()[-1] for l in lines if l.startswith("property float")]
    vert = np.frombuffer(body[:nv * 4 * len(props)], dtype="<f4").reshape(nv, len(props))
    rec = np.frombuffer(body[nv * 4 * len(props):], dtype=[("count", "u1"), ("index", "<i4", 3)])
    assert rec.shape[0] == nf and (rec["count"] == 3).all()
    return vert, rec["index"], props


@pytest.mark.parametrize("normals", [True, False])
def test_obj_round_trip(tmp_path, normals):
    m = small_mesh(normals)
    v, f, n = read_obj(m.export(str(tmp_path / "m.obj")))
    assert np.array_equal(v, m.vertices) and np.array_equal(f, m.faces)
    assert (np.array_equal(n, m.vertex_normals)) if normals else n.size == 0


def test_stl_round_trip_up_to_its_unwelded_layout(tmp_path):
    m = small_mesh()
    normal, corners = read_stl(m.export(str(tmp_path / "m.stl")))
    assert np.array_equal(corners, m.vertices[m.faces])
    assert np.allclose(normal, m.face_normals, atol=1e-6)


@pytest.mark.parametrize("normals", [True, False])
def test_ply_round_trip(tmp_path, normals):
    m = small_mesh(normals)
    vert, faces, props = read_ply(m.export(str(tmp_path / "m.ply")))
    assert props == ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else [])
    assert np.array_equal(vert[:, :3], m.vertices) and np.array_equal(faces, m.faces)
    if normals:
        assert np.array_equal(vert[:, 3:], m.vertex_normals)


def test_unknown_extension_is_refused(tmp_path):
    with pytest.raises(ValueError):
        small_mesh().export(str(tmp_path / "m.off"))


def test_transform_and_translation_are_the_numpy_formulas():
    rng = np.random.RandomState(5)
    q, _ = np.linalg.qr(rng.randn(3, 3))
    for rot in (q if np.linalg.det(q) > 0 else -q, q if np.linalg.det(q) < 0 else -q, np.diag([2.0, 0.5, 1.5])):
        m = small_mesh()
        v0, n0, f0 = m.vertices.astype(np.float64), m.vertex_normals.astype(np.float64), m.faces.copy()
        mat = np.eye(4)
        mat[:3, :3] = rot
        mat[:3, 3] = [0.25, -1.5, 3.0]
        assert m.apply_transform(mat) is m
        want_v = (np.concatenate([v0, np.ones((6, 1))], axis=1) @ mat.T)[:, :3]
        want_n = n0 @ rot.T
        want_n /= np.linalg.norm(want_n, axis=1, keepdims=True)
        assert m.vertices.dtype == np.float32 and np.array_equal(m.vertices, want_v.astype(np.float32))
        assert np.allclose(m.vertex_normals, want_n, atol=1e-6)
        assert np.array_equal(m.faces, f0[:, ::-1] if np.linalg.det(rot) < 0 else f0)
    m = small_mesh()
    v0 = m.vertices.astype(np.float64)
    assert m.apply_translation([1.0, -2.0, 0.5]) is m
    assert np.array_equal(m.vertices, (v0 + [1.0, -2.0, 0.5]).astype(np.float32))
    with pytest.raises(ValueError):
        m.apply_transform(np.eye(3))
