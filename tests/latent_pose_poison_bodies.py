"""Poison-tier bodies of the pose fit (tests/poison.py): sg_sdfnet_latent_pose_grad writes every row of its tile partials in full —
ragged last tiles, table rows that name nothing and floats 526 / 527 included —, sg_sdfnet_latent_pose_reduce every element of t1, t5,
loss and gpose (floats 13..15 too); nothing stale is read; two runs are bit-identical; a small call right after a large one equals the
small call alone; the whole fit runs under poison."""
import numpy as np
import torch

import latent_pose_forms as F
from poison import poisoned

RUNS = (1, 31, 33, 65, 200, 2)      # one lane, a tile less one, a tile and one, two tiles and one, seven tiles less 24, two lanes
FORMS = ((None, 0.0), ((0, 40), 0.01), ((190, 64), 0.01))      # window, sigma


def _case():
    return F.make_case("seeded", 29, RUNS, 190, 0.01, "affine")


def snapshot(dev, window, sigma):
    case = _case()
    net = F.net_on(dev, case.seed, case.latent, case.sd)
    out = F.run(net, dev, case.pts, case.tgt, case.z, case.pose, case.seg_off, cutoff=F.CUTOFF, sigma=sigma, window=window)
    return tuple(o.clone() for o in out)


def check_outputs_and_repeat(dev, window, sigma):
    plain = snapshot(dev, window, sigma)
    with poisoned() as p:
        first = snapshot(dev, window, sigma)
        p.renew()
        second = snapshot(dev, window, sigma)
        p.check_canaries()
    for got in (first, second):
        for o, q in zip(got, plain):
            assert not torch.isnan(o).any(), "an output element was not written"
            assert torch.equal(o, q)
        assert torch.equal(got[2][:, 13:], torch.zeros(len(RUNS), 3)), "floats 13..15 of grad_pose"


def check_raw_rows(dev):
    """The entry points themselves on NaN-filled buffers, with table rows that name nothing among the real ones: every float of every
    row, and of t1, t5, loss and gpose, is written; the rows that name nothing are zeros and change no other row."""
    from shapegan_amd import ops
    case = _case()
    net, plain, _ = F._fit_objects(dev, case)
    lib = ops._lib()
    S = len(RUNS)
    _, _, tiles, tile_off, ntiles = plain._plan(0)[0]
    z, pose = case.z.to(dev), case.pose.to(dev)
    w1, b1, w5, b5 = plain.params[0], plain.params[1], plain.params[8], plain.params[9]
    zb1, zb5 = torch.zeros(S, 256, device=dev), torch.zeros(S, 256, device=dev)
    ops.check(lib.sg_sdfnet_shape_bias(ops.ptr(z), S, case.latent, ops.ptr(w1), ops.ptr(b1), ops.ptr(w5), ops.ptr(b5), ops.ptr(zb1),
                                       ops.ptr(zb5), ops.stream()), "shape_bias")

    def grad(table):
        part = torch.full((table.shape[0], 528), float("nan"), device=dev)
        ops.check(lib.sg_sdfnet_latent_pose_grad(ops.ptr(plain.points), ops.ptr(plain.sdf), ops.ptr(plain.seg_off), S, ops.ptr(zb1),
                                                 ops.ptr(zb5), ops.ptr(plain.packed), ops.ptr(pose), F.CUTOFF, 0, 0, ops.ptr(table),
                                                 table.shape[0], ops.ptr(part), ops.stream()), "latent_pose_grad")
        return part
    real = grad(tiles)
    assert real.shape[0] == ntiles and not torch.isnan(real).any(), "an element of a partial row was not written"
    assert torch.equal(real[:, 526:], torch.zeros(ntiles, 2, device=dev)), "floats 526 / 527"
    nothing = torch.tensor([[-1, 0], [S, 0], [4, -32], [4, 224], [0, 32], [2, 1 << 20]], dtype=torch.int32, device=dev)
    mixed = torch.cat([nothing[:3], tiles, nothing[3:]])
    got = grad(mixed)
    assert not torch.isnan(got).any(), "a row that names nothing was not written in full"
    assert torch.equal(got[:3], torch.zeros(3, 528, device=dev)) and torch.equal(got[3 + ntiles:], torch.zeros(3, 528, device=dev))
    assert torch.equal(got[3:3 + ntiles], real), "the rows of the real tiles depend on the rest of the table"
    outs = [torch.full(shape, float("nan"), device=dev) for shape in ((256, S), (256, S), (S,), (S, 16))]
    ops.check(lib.sg_sdfnet_latent_pose_reduce(ops.ptr(real), ops.ptr(tile_off), ops.ptr(plain.seg_off), S, 0, *[ops.ptr(o) for o in outs],
                                               ops.stream()), "latent_pose_reduce")
    for o, name in zip(outs, ("t1", "t5", "loss", "gpose")):
        assert not torch.isnan(o).any(), "an element of %s was not written" % name
    assert torch.equal(outs[3][:, 13:], torch.zeros(S, 3, device=dev)), "floats 13..15 of gpose"
    # gpose is the tiles' sums in pose's layout, added in double in tile order
    to = tile_off.cpu().numpy()
    rows = real.double().cpu().numpy()
    for s in range(S):
        acc = np.zeros(16)
        for t in range(to[s], to[s + 1]):
            r = rows[t]
            acc[:12] += np.concatenate([r[513:522].reshape(3, 3), r[522:525].reshape(3, 1)], axis=1).reshape(12)
            acc[12] += r[525]
        assert np.array_equal(acc.astype(np.float32), outs[3][s].cpu().numpy()), "gpose of shape %d is not its tiles' sums in tile order" % s


def check_small_after_large(dev):
    """The large call's partials lie where the small call's will (the allocator hands the block back): the small call must not see them."""
    big = F.make_case("seeded", 29, (300, 300, 300), 191, 0.01, "affine")
    case = _case()
    net = F.net_on(dev, case.seed, case.latent, case.sd)
    so = case.seg_off.tolist()
    small = (case.pts[so[3]:so[4]], case.tgt[so[3]:so[4]], case.z[3:4], case.pose[3:4], torch.tensor([0, so[4] - so[3]]))
    large = (big.pts, big.tgt, case.z[:3], big.pose, big.seg_off)
    alone = F.run(net, dev, *small, cutoff=F.CUTOFF, sigma=0.01)
    with poisoned() as p:
        F.run(net, dev, *large, cutoff=F.CUTOFF, sigma=0.01)
        after = F.run(net, dev, *small, cutoff=F.CUTOFF, sigma=0.01)
        p.check_canaries()
    F._same(after, alone, "small call after a large one, under poison")
    F.run(net, dev, *large, cutoff=F.CUTOFF, sigma=0.01)
    F._same(F.run(net, dev, *small, cutoff=F.CUTOFF, sigma=0.01), alone, "small call after a large one")


def check_fit_under_poison(dev):
    from shapegan_amd.reconstruct import fit_codes_and_poses
    case = _case()
    net = F.net_on(dev, case.seed, case.latent, case.sd)
    kw = dict(iterations=3, lr=1e-3, pose_lr=1e-3, points_per_step=40, seed=1, rotation_starts=2)
    plain = fit_codes_and_poses(net, case.pts.to(dev), case.tgt.to(dev), case.seg_off.to(dev), **kw)
    with poisoned() as p:
        codes, poses, loss = fit_codes_and_poses(net, case.pts.to(dev), case.tgt.to(dev), case.seg_off.to(dev), **kw)
        p.check_canaries()
    assert torch.equal(codes.cpu(), plain[0].cpu()) and torch.equal(loss.cpu(), plain[2].cpu())
    assert torch.equal(poses.theta.cpu(), plain[1].theta.cpu()) and torch.equal(poses.matrix.cpu(), plain[1].matrix.cpu())
    assert not torch.isnan(poses.matrix).any() and not torch.isnan(poses.scale).any()
