"""Mesh simplification on the GPU (csrc/simplify.hip): every case of tests/simplify_cases.py against the twin, bit for bit, and against the
numpy reference; marching-cubes batches with empty shapes at every position; one cluster that owns many tiles of corner records."""
import numpy as np
import pytest
import torch

import simplify_cases as K
import simplify_poison_bodies as B
from shapegan_amd import simplify as SM
from shapegan_amd.mesh import marching_cubes

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", sorted(K.CASES))
def test_cases_against_the_twin_and_the_reference(case):
    name, kw = K.CASES[case]
    got, worst = K.check_case_against_reference(case, DEV)
    twin, info_twin = SM.simplify_meshes(K.built(name), **kw)
    assert K.same_batches(got, twin)
    again, info = SM.simplify_meshes(K.built(name, DEV), **kw)
    assert K.same_batches(again, got)
    for k in info:
        assert torch.equal(info[k], info_twin[k]), k


@pytest.fixture(scope="module")
def mixed():
    """test_gpu_mesh.mixed_batch(24, 32, seed) with empty shapes first, in the middle and last: on the GPU and, copied, for the twin."""
    from test_gpu_mesh import mixed_batch
    grids = mixed_batch(24, 32, 5)
    grids[0] = grids[12] = grids[23] = 1.0
    h = 2.0 / 31
    gpu = marching_cubes(grids.to(DEV), level=0.0, spacing=h, origin=-1.0 - h, pad=True, pad_value=1.0)
    counts = gpu.triangle_counts().tolist()
    assert counts[0] == counts[12] == counts[23] == 0 and min(c for i, c in enumerate(counts) if i not in (0, 12, 23)) > 0
    return gpu, K.to_device(gpu, "cpu")


@pytest.mark.parametrize("kw", [{"cells": 8}, {"cells": 1}, {"cells": 8, "placement": "mean"}, {"cell": 0.17}, {"target_triangles": 400}],
                         ids=["cells8", "cells1", "mean", "cell", "target"])
def test_marching_cubes_batch_against_the_twin_and_repeated(mixed, kw):
    gpu, cpu = mixed
    got, info = SM.simplify_meshes(gpu, **kw)
    twin, info_twin = SM.simplify_meshes(cpu, **kw)
    assert K.same_batches(got, twin) and K.same_batches(SM.simplify_meshes(gpu, **kw)[0], got)
    for k in info:
        assert torch.equal(info[k], info_twin[k]), k
    after = info["triangles_after"]
    assert after[0] == after[12] == after[23] == 0
    if kw.get("cells") == 1:
        assert int(after.sum()) == 0 and got.vertices.shape[0] == 0
    elif "target_triangles" in kw:
        assert (after <= 400).all() and int(after.sum()) > 0
    else:
        assert 0 < int(after.sum()) < int(info["triangles_before"].sum())


def test_a_shape_does_not_depend_on_its_batch_with_cell():
    ico, cube, sphere = K.built("icosphere", DEV), K.built("cube", DEV), K.built("sphere16", DEV)
    kw = {"cell": 0.21, "origin": (-1.0, -1.0, -1.0)}
    alone = SM.simplify_meshes(ico, **kw)[0]
    assert alone.faces.shape[0] > 100 and K.same_batches(alone, SM.simplify_meshes(K.built("icosphere"), **kw)[0])
    for order in ([ico, cube, sphere], [cube, ico, sphere], [cube, sphere, ico]):
        got = SM.simplify_meshes(K.concat(order), **kw)[0]
        assert K.same_batches(K.shape_of(got, order.index(ico)), alone)


@pytest.mark.parametrize("cells", [1, 2])
def test_one_cluster_with_many_tiles_of_corner_records(cells):
    """At one cell the icosphere's single cluster owns all 2562 vertices (41 tiles) and one corner record of each of its 5120 triangles
    (80 tiles); at two cells eight clusters own some 700 records each.  The cluster table, which the final mesh does not show at
    one cell, equals the twin's bit for bit and lies inside the cells."""
    gpu = B.stages(K.built("icosphere", DEV), {"cells": cells})
    cpu = B.stages(K.built("icosphere"), {"cells": cells})
    assert gpu[-1] == cpu[-1] and gpu[4].shape == (cells ** 3, 3)
    for g, c in zip(gpu[:-1], cpu[:-1]):
        g = g.cpu()
        if g.dtype == torch.float32:
            g, c = g.contiguous().view(torch.int32), c.contiguous().view(torch.int32)
        assert torch.equal(g, c)
    records = gpu[3].cpu().reshape(-1)
    assert int((records != 2 ** 63 - 1).sum()) >= 5120
    table = gpu[4].cpu().numpy()
    assert np.isfinite(table).all() and np.abs(table).max() <= 0.81
