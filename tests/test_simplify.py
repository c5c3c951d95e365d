"""Mesh simplification on the C++ twin (shapegan_amd/simplify.py, csrc/simplify_core.h) against the numpy reference
(tests/simplify_reference.py), by hand-built meshes with known answers, and through get_mesh, reconstruct_meshes and the command line."""
import numpy as np
import pytest
import torch

import simplify_cases as K
import simplify_reference as R
from shapegan_amd import simplify as SM
from shapegan_amd import topology as T
from shapegan_amd.mesh import Mesh, MeshBatch


@pytest.mark.parametrize("case", sorted(K.CASES))
def test_against_the_reference(case):
    K.check_case_against_reference(case, "cpu")


def hand(name, **kw):
    batch = K.pack([K.hand_meshes()[name]])
    return batch, SM.simplify_meshes(batch, **kw)


def test_one_triangle_survives_whole_or_not_at_all():
    batch, (got, info) = hand("one_triangle", cells=4)
    assert got.faces.tolist() == [[0, 1, 2]] or sorted(got.faces[0].tolist()) == [0, 1, 2]
    assert got.vertices.shape == (3, 3) and info["triangles_after"].tolist() == [1]
    # the quadric of a single plane leaves the mean where it is: the three vertices come back (within float32 of their own cell)
    order = got.faces[0].tolist()
    assert np.allclose(got.vertices.numpy()[order], batch.vertices.numpy(), atol=1e-6)
    got, info = SM.simplify_meshes(batch, cells=1)
    assert got.faces.shape == (0, 3) and got.vertices.shape == (0, 3) and info["triangles_after"].tolist() == [0]


def test_tetrahedron_collapses_at_one_cell_and_is_kept_at_four():
    batch, (got, info) = hand("tetrahedron", cells=1)
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.vert_offsets.tolist() == [0, 0]
    got, info = SM.simplify_meshes(batch, cells=4)
    # nothing merges: the output is the input up to the renumbering by cell (z fastest: vertex 3 = (0, 0, 1) comes second)
    assert info["triangles_after"].tolist() == [4] and got.vertices.shape == (4, 3)
    perm = [0, 3, 2, 1]      # old vertex -> new index, from the key order (0,0,0) < (0,0,3) < (0,3,0) < (3,0,0)
    assert got.faces.tolist() == [[perm[i] for i in tri] for tri in K.TET_F.tolist()]
    assert np.allclose(got.vertices.numpy()[perm], K.TET_V, atol=1e-6)
    for placement in ("quadric", "mean"):
        assert SM.simplify_meshes(batch, cells=4, placement=placement)[0].faces.tolist() == got.faces.tolist()
    assert torch.equal(SM.simplify_meshes(batch, cells=4, placement="mean")[0].vertices[perm], batch.vertices)      # a mean of one


def test_opposite_normals_in_one_cell_give_a_zero_normal():
    batch, (got, _) = hand("opposite_normals", cells=2)
    assert got.vertices.shape[0] == 4      # vertices 0 and 1 merged
    assert got.normals[0].tolist() == [0.0, 0.0, 0.0] and (got.normals[1:].norm(dim=1) - 1).abs().max() < 1e-6


def test_unreferenced_vertices_and_skipped_triangles_leave_no_trace():
    for name in ("unreferenced_vertex", "out_of_range"):
        batch, (got, info) = hand(name, cells=4)
        assert info["triangles_after"].tolist() == [4] and got.vertices.shape[0] == 4
        assert sorted(got.faces.reshape(-1).tolist()) == sorted([0, 1, 2, 3] * 3)


def test_zero_area_triangle_adds_nothing_to_the_quadrics():
    h = K.hand_meshes()
    with_it = K.pack([h["zero_area"]])
    v, f, _ = h["zero_area"]
    without = K.pack([(v, f[:-1], with_it.normals.numpy())])
    a, b = SM.simplify_meshes(with_it, cells=1), SM.simplify_meshes(without, cells=1)
    assert K.same_batches(a[0], b[0])
    # at cells = 4 the degenerate triangle survives as a triangle (three cells) and the positions of its corners are those without it
    a, b = SM.simplify_meshes(with_it, cells=4)[0], SM.simplify_meshes(without, cells=4)[0]
    # (its middle vertex, alone in cell (2, 2, 0), is vertex 3 of the five in key order)
    assert a.faces.shape[0] == b.faces.shape[0] + 1 and a.vertices.shape[0] == b.vertices.shape[0] + 1
    assert torch.equal(a.vertices[[0, 1, 2, 4]].view(torch.int32), b.vertices.view(torch.int32))


def test_nan_coordinate_goes_to_cell_zero_and_stays_local():
    batch, (got, info) = hand("nan_coordinate", cells=4)
    ref = R.simplify(batch, cells=4)
    R.check_against(got, ref, left_out=1.0)
    assert int(ref["keys"][4]) == (0 << 28) | (2 << 14) | 2      # x is NaN: cell 0 along x; y = z = 0.5 of 1: cell 2 of 4
    bad = torch.isnan(got.vertices).any(dim=1)
    assert 0 < int(bad.sum()) < got.vertices.shape[0]
    assert (got.vertices.view(torch.int32)[torch.isnan(got.vertices)] == 0x7fc00000).all()      # one NaN, the same everywhere


def test_a_shape_without_triangles_between_two_others():
    h = K.hand_meshes()
    batch = K.pack([h["tetrahedron"], h["no_triangles"], (h["tetrahedron"][0] + 2, h["tetrahedron"][1], None)])
    got, info = SM.simplify_meshes(batch, cells=4)
    assert got.tri_offsets.tolist() == [0, 4, 4, 8] and got.vert_offsets.tolist() == [0, 4, 4, 8]
    assert torch.equal(got.faces[:4], got.faces[4:])
    R.check_against(got, R.simplify(batch, cells=4), left_out=1.0)


def test_cube_keeps_its_volume_and_stays_watertight():
    got, _ = K.check_case_against_reference("cube-3")
    s = T.components(got).summary()
    assert got.faces.shape[0] == 48 and s["watertight"].tolist() == [True] and s["components"].tolist() == [1]
    assert float(s["volume"][0]) == pytest.approx(R.volume(K.reference("cube-3")["positions"], K.reference("cube-3")["faces"]), abs=1e-6)
    # the reference's own numbers, taken at run time: the quadric placement loses less than a quarter of what the mean loses
    quadric, mean = K.reference("cube-3"), K.reference("cube-3-mean")
    err_q, err_m = abs(R.volume(quadric["positions"], quadric["faces"]) - 1), abs(R.volume(mean["positions"], mean["faces"]) - 1)
    print("[simplify] cube at 3 cells: volume error quadric %.5f, mean %.5f" % (err_q, err_m))
    assert err_q < 0.25 * err_m


def test_icosphere_volume_quadric_beats_mean():
    true = 4 / 3 * np.pi * 0.8 ** 3
    q, m = K.reference("icosphere-6"), K.reference("icosphere-6-mean")
    assert abs(R.volume(q["positions"], q["faces"]) - true) < abs(R.volume(m["positions"], m["faces"]) - true)


def test_a_shape_does_not_depend_on_its_batch_with_cell():
    ico, cube, sphere = K.built("icosphere"), K.built("cube"), K.built("sphere16")
    kw = {"cell": 0.21, "origin": (-1.0, -1.0, -1.0)}
    alone = SM.simplify_meshes(ico, **kw)[0]
    assert alone.faces.shape[0] > 100
    for order in ([ico, cube, sphere], [cube, ico, sphere], [cube, sphere, ico]):
        got = SM.simplify_meshes(K.concat(order), **kw)[0]
        assert K.same_batches(K.shape_of(got, order.index(ico)), alone)


def test_target_triangles():
    got, info = SM.simplify_meshes(K.built("icosphere"), target_triangles=500)
    assert 0 < int(info["triangles_after"][0]) <= 500 and int(info["cells"][0]) == int(K.reference("icosphere-target")["cells"][0])
    batch = K.built("mixed")
    targets = [500, 5, 100, 10, 0]
    got, info = SM.simplify_meshes(batch, target_triangles=targets)
    assert (info["triangles_after"] <= torch.tensor(targets)).all()
    assert info["cells"].tolist() == K.reference("mixed-target")["cells"].tolist()
    # the tetrahedron already fits: it comes back unchanged, bit for bit, its unreferenced nothing included
    assert info["cells"][3] == 0 and K.same_batches(K.shape_of(got, 3), K.shape_of(batch, 3))
    assert K.same_batches(SM.simplify_meshes(batch, target_triangles=10 ** 6)[0], batch)


def test_refusals_come_before_any_launch(monkeypatch):
    batch = K.built("cube")
    monkeypatch.setattr(SM.L, "load", lambda: (_ for _ in ()).throw(AssertionError("a library call was made")))
    with pytest.raises(ValueError):
        SM.simplify_meshes(batch, cells=16385)
    with pytest.raises(ValueError):
        SM.simplify_meshes(batch, cells=0)
    for h in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            SM.simplify_meshes(batch, cell=h)
    with pytest.raises(ValueError):
        SM.simplify_meshes(batch, cell=0.1, cells=4)
    with pytest.raises(ValueError):
        SM.simplify_meshes(batch)
    with pytest.raises(ValueError):
        SM.simplify_meshes(batch, cells=4, placement="median")
    with pytest.raises(ValueError):
        SM.simplify_meshes(batch, target_triangles=-1)


def test_the_entry_points_refuse_sizes_beyond_the_key():
    lib = SM.L.load()
    assert lib.sg_simplify_clusters_workspace_bytes(1 << 20, 10) == 0 and lib.sg_simplify_clusters_workspace_bytes(1, 1 << 31) == 0
    assert lib.sg_simplify_faces_workspace_bytes(1, 10, 1 << 31) == 0 and lib.sg_simplify_faces_workspace_bytes((1 << 20) - 1, 10, 10) > 0
    keys = torch.empty(4, dtype=torch.int64)
    b = K.pack([K.hand_meshes()["tetrahedron"]])
    grid = SM._Grid(np.zeros((1, 3)), np.ones(1), np.ones(1)).upload("cpu")
    try:
        rc = lib.sg_simplify_keys(SM.ptr(b.vertices), SM.ptr(b.vert_offsets), 1 << 20, 4, SM.ptr(grid[0]), SM.ptr(grid[1]), SM.ptr(grid[2]),
                                  SM.ptr(keys), None)
    finally:
        SM.L.reset_call_state()
    assert rc != 0


def test_mesh_and_batch_methods():
    v, f, n = K.cube()
    mesh = Mesh(v, f, n)
    small = mesh.simplify(cells=3)
    want = SM.simplify_meshes(K.built("cube"), cells=3)[0].mesh(0)
    assert np.array_equal(small.vertices, want.vertices) and np.array_equal(small.faces, want.faces)
    assert np.array_equal(small.vertex_normals, want.vertex_normals) and small.is_watertight
    assert Mesh(v, f).simplify(target_triangles=100).vertex_normals is None
    assert K.same_batches(K.built("cube").simplify(cells=3), SM.simplify_meshes(K.built("cube"), cells=3)[0])
    assert SM.simplify_option(None) is None and SM.simplify_option(False) is None and SM.simplify_option(300) == {"target_triangles": 300}
    assert SM.simplify_option({"cells": 8}) == {"cells": 8}
    with pytest.raises(ValueError):
        SM.simplify_option(True)


# ---- through the network: get_mesh, reconstruct_meshes, the command line (on the twin) ----------------------------------------------------
RES = 32


@pytest.fixture(scope="module")
def chairs():
    import project_forms
    net = project_forms.chairs_net("cpu")[0]
    codes = torch.stack([torch.randn(128, generator=torch.Generator().manual_seed(s)) for s in (0, 1)])
    return net, codes


def test_get_mesh_simplify(chairs):
    net, codes = chairs
    plain = net.get_mesh(codes[0], RES)
    assert np.array_equal(net.get_mesh(codes[0], RES, simplify=None).vertices, plain.vertices)
    for option in (200, {"cells": 12}, {"cell": 0.1, "placement": "mean"}):
        got = net.get_mesh(codes[0], RES, simplify=option)
        want = plain.simplify(**SM.simplify_option(option))
        assert np.array_equal(got.vertices, want.vertices) and np.array_equal(got.faces, want.faces)
        assert np.array_equal(got.vertex_normals, want.vertex_normals) and 0 < len(got.faces) < len(plain.faces)
    assert len(net.get_mesh(codes[0], RES, simplify=200).faces) <= 200


def test_reconstruct_meshes_simplify_comes_last(chairs):
    from shapegan_amd.reconstruct import reconstruct_meshes
    from shapegan_amd.surface import cell_diagonal, refine_meshes
    net, codes = chairs
    plain = reconstruct_meshes(net, codes, RES)
    assert K.same_batches(reconstruct_meshes(net, codes, RES, simplify=None), plain)
    refined = refine_meshes(net, codes, T.clean_meshes(plain, "largest")[0], iterations=1, max_move=cell_diagonal(RES))[0]
    want, info = SM.simplify_meshes(refined, target_triangles=300)
    got = reconstruct_meshes(net, codes, RES, clean="largest", refine=1, simplify=300)
    assert K.same_batches(got, want) and (info["triangles_after"] <= 300).all() and (info["triangles_after"] > 0).all()


TETRAHEDRA = """v 0 0 0
v 1 0 0
v 0 1 0
v 0 0 1
f 1 3 2
f 1 2 4
f 1 4 3
f 2 3 4
v 2 2 2
v 3 2 2
v 2 3 2
v 2 2 3
f 5 7 6
f 5 6 8
f 5 8 7
f 6 7 8
"""


def test_command_line_simplify(tmp_path, chairs_state, capsys):
    from shapegan_amd import prepare, reconstruct
    models = tmp_path / "models" / "abc" / "models"
    models.mkdir(parents=True)
    (models / "model_normalized.obj").write_text(TETRAHEDRA)
    torch.save(chairs_state, str(tmp_path / "sdf_net.to"))
    argv = ["--net", str(tmp_path / "sdf_net.to"), "--models", str(tmp_path / "models"), "--out", str(tmp_path / "codes.to"), "--device", "cpu",
            "--points", "300", "--iterations", "2", "--scan-count", "6", "--scan-resolution", "64", "--resolution", "16"]
    assert reconstruct.main(argv + ["--meshes", str(tmp_path / "plain")]) == 0
    assert reconstruct.main(argv + ["--meshes", str(tmp_path / "small"), "--simplify", "60"]) == 0
    capsys.readouterr()
    pv, pf = prepare.load_obj(str(tmp_path / "plain" / "0000.obj"))
    sv, sf = prepare.load_obj(str(tmp_path / "small" / "0000.obj"))
    assert len(pf) > 60 and 0 < len(sf) <= 60
    # the file is write_obj of the simplified reconstruction of the fitted codes
    from shapegan_amd.model.sdf_net import SDFNet
    net = SDFNet(device="cpu")
    net.load_state_dict(chairs_state)
    SM.L.bump_param_epoch()
    want = reconstruct.reconstruct_meshes(net, torch.load(str(tmp_path / "codes.to")), 16, simplify=60)
    reconstruct.write_obj(str(tmp_path / "want.obj"), want.mesh(0))
    assert (tmp_path / "want.obj").read_text() == (tmp_path / "small" / "0000.obj").read_text()
