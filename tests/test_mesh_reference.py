"""Marching cubes and surface sampling on the C++ twin against the direct numpy / float64 references of
tests/geometry_reference.py (written from include/shapegan_hip.h, K12; faces from scripts/gen_mc_tables.py's generator, not from
csrc/mc_tables.h); tests/test_gpu_mesh.py runs the same bodies on the MI355X."""
import pytest
import torch

import geometry_reference as R
from shapegan_amd.mesh import marching_cubes, sample_packed

DEVICE = "cpu"


def mesh(grids, dev, level, pad, pad_value):
    return marching_cubes(grids.to(dev), level=level, spacing=R.MC_SPACING, origin=R.MC_ORIGIN, pad=pad, pad_value=pad_value)


def body_mc(dev, shape, S=3, combos=None):
    """Every (pad, level, pad_value) of the case list on a batch of `shape`; returns the figures and the batches."""
    worst = dict(pos_err=0.0, pos_bound=0.0, normal_err=0.0, normal_ratio=0.0, verts=0, tris=0)
    done = []
    for pad in (True, False):
        for i, (level, pad_value) in enumerate(R.MC_LEVELS):
            if combos is not None and (pad, i) not in combos:
                continue
            grids = R.mc_batch(shape, level, pad_value, seed=100 + 10 * i + sum(shape), S=S)
            batch = mesh(grids, dev, level, pad, pad_value)
            out = R.check_mc(batch, grids, level, pad, pad_value)
            for k in worst:
                worst[k] = max(worst[k], out[k]) if k.endswith(("err", "bound", "ratio")) else worst[k] + out[k]
            done.append((grids, dict(level=level, pad=pad, pad_value=pad_value), batch))
    print("marching cubes", shape, S, worst)
    return worst, done


def test_case_table_points_toward_increasing_values():
    R.check_case_table_orientation()


@pytest.mark.parametrize("shape", R.MC_SHAPES)
def test_marching_cubes_against_reference(shape):
    worst, _ = body_mc(DEVICE, shape)
    if min(shape) >= 2:
        assert worst["verts"] > 0 and worst["tris"] > 0


def test_marching_cubes_many_blocks():
    # 35 * 34 * 33 padded corners are 154 workgroups of 256 per grid: 3 grids stay below the 1,024 scan threads, 7 go beyond
    body_mc(DEVICE, (33, 32, 31), S=7, combos={(True, 0)})


def body_sampling(dev):
    samples = fragile = 0
    worst = 0.0
    grids = R.mc_batch((16, 16, 17), 0.0, 1.0, seed=50, S=4)       # noise, blank, noise with corners at the level, noise
    batch = mesh(grids, dev, 0.0, True, 1.0)
    packs = [(batch.vertices, batch.faces, batch.vert_offsets, batch.tri_offsets, [0, 1, 0, 0]),
             tuple(t.to(dev) for t in R.hand_mesh()) + ([0, 1, 0],)]
    for v, f, vo, to, empty_want in packs:
        for P in (1, 255, 4097):
            S = len(empty_want)
            u = R.special_uniforms(torch.rand((S, P, 3), generator=torch.Generator().manual_seed(P)))
            pts, empty = sample_packed(v, f, vo, to, u.to(dev))
            assert empty.tolist() == empty_want
            out = R.check_sampling(R.npy(v), R.npy(f), R.npy(vo), R.npy(to), R.npy(u), R.npy(pts), R.npy(empty))
            samples, fragile, worst = samples + out["samples"], fragile + out["fragile"], max(worst, out["err_ratio"])
    assert fragile <= R.SAMPLE_FRAGILE_CAP * samples, (fragile, samples)
    print("sampling", dict(samples=samples, fragile=fragile, err_ratio=worst))
    return samples, fragile, worst


def test_surface_sampling_against_reference():
    body_sampling(DEVICE)
