"""Poison-tier bodies of the mesh-to-SDF entry points (tests/poison.py): every output element written, indices in range, canaries
intact, two runs bit-identical, and a small call right after a large one equal to the twin's result for the small call alone.

The distance kernel's workspace ("meshsdf") holds the triangle records and, behind them, the packed minima (bits(d2) << 32 | index) of
the triangle split, whose low halves BECOME the indices `tri` and select the record `closest` is computed from.  poison.INDEX_WORKSPACES
does not list it, so under poison it is filled with 0xFF bytes — which is also the state the entry point itself puts the words in
(hipMemsetAsync) before the launch: the result does not depend on what the workspace held, which the small-after-large body and the
bit-identical repeat (renew() leaves 0x7F bytes behind) assert.
"""
import numpy as np
import torch

from shapegan_amd import prepare as P
from poison import poisoned
import prepare_reference as R
import test_prepare as T

FORMS = ((65, 300), (5, 3000), (1000, 775))      # one query per lane; the triangle split; four queries per lane, several chunks


def snapshot(device, Q, T_):
    """numpy copies (renew() may scribble over the tensors): distance with every output, then sdf and outside."""
    tris, points = T.form_case(Q, T_)
    dist2, tri, closest, _ = T.run_distance([tris, tris[:T_ // 2]], np.concatenate([points, points[:, ::-1]]), device)
    depth, vps = T.rule_scan(device)
    p = torch.from_numpy(np.concatenate([points, points[:, ::-1]])).to(device)
    sdf, outside = P.mesh_sign(p, depth.expand(1, 2, 4, 4).contiguous(), vps, 0.25, dist2=torch.from_numpy(dist2).to(device))
    return dist2.copy(), tri.copy(), closest.copy(), sdf.cpu().numpy().copy(), outside.cpu().numpy().copy()


def check_outputs_and_repeat(device, Q, T_):
    plain = snapshot(device, Q, T_)
    with poisoned() as p:
        first = snapshot(device, Q, T_)
        p.renew()
        second = snapshot(device, Q, T_)
        p.check_canaries()
    for got in (first, second):
        dist2, tri, closest, sdf, outside = got
        assert not np.isnan(dist2).any() and not np.isnan(sdf).any() and not np.isnan(closest).any(), "NaN left"
        assert (tri[0] >= 0).all() and (tri[0] < T_).all() and (tri[1] >= 0).all() and (tri[1] < T_ // 2).all()
        assert (outside <= 1).all()
        for x, y in zip(got, plain):
            np.testing.assert_array_equal(x, y)


def check_small_after_large(device):
    """The packed minima of a large call lie where a small call's will: the small call must not see them."""
    big_tris, big_points = T.form_case(1000, 775)
    tris, points = T.form_case(63, 40)
    alone = T.run_distance([tris], points, "cpu")
    with poisoned() as p:
        T.run_distance([big_tris], big_points, device)
        after = T.run_distance([tris], points, device)
        p.check_canaries()
    T.assert_same_bits(after[:3], alone[:3])
    # KEEP: this is the one assertion that fails when the entry point stops setting the packed minima itself.  Under poison the
    # scratch is 0xFF bytes, which is exactly that initial state, so the poisoned runs above cannot see a missing fill; here the cached
    # workspace really is the large call's, and the small call's words lie over the large call's triangle records.
    T.run_distance([big_tris], big_points, device)
    T.assert_same_bits(T.run_distance([tris], points, device)[:3], alone[:3])


def check_pipeline_under_poison(device):
    """SurfaceScans end to end: every voxel and every cloud value written."""
    with poisoned() as p:
        scans = P.SurfaceScans([R.mesh("box"), R.mesh("torus")], 3 ** 0.5, 6, 32, device=device)
        voxels, ok = scans.get_voxels(8, check_result=True)
        points, sdf, good = scans.sample_sdf_near_surface(500, generator=torch.Generator().manual_seed(1))
        p.check_canaries()
    assert not torch.isnan(voxels).any() and not torch.isnan(sdf).any() and not torch.isnan(points).any()
    assert ok.tolist() == [True, True]
