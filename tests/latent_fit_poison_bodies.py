"""Poison-tier bodies of the latent fit (tests/poison.py): sg_sdfnet_latent_grad writes every row of its tile partials in full, ragged
last tiles included, sg_sdfnet_latent_reduce and the fold's backward every output element; nothing stale is read; two runs are
bit-identical; a small call right after a large one equals the small call alone."""
import torch

import latent_fit_forms as F
from poison import poisoned

RUNS = (1, 31, 33, 65, 200, 2)      # one lane, a tile less one, a tile and one, two tiles and one, seven tiles less 24, two lanes
FORMS = ((None, 0.0), ((0, 40), 0.01), ((190, 64), 0.01))      # window, sigma


def _case():
    return F.make_case("seeded", 29, RUNS, 90, 0.01)


def snapshot(dev, window, sigma):
    case = _case()
    net = F.net_on(dev, case.seed, case.latent, case.sd)
    loss, grad = F.run(net, dev, case.pts, case.tgt, case.z, case.seg_off, cutoff=F.CUTOFF, sigma=sigma, window=window)
    return loss.clone(), grad.clone()


def check_outputs_and_repeat(dev, window, sigma):
    plain = snapshot(dev, window, sigma)
    with poisoned() as p:
        first = snapshot(dev, window, sigma)
        p.renew()
        second = snapshot(dev, window, sigma)
        p.check_canaries()
    for got in (first, second):
        assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any(), "an output element was not written"
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])


def check_small_after_large(dev):
    """The large call's partials lie where the small call's will (the allocator hands the block back): the small call must not see them."""
    big = F.make_case("seeded", 29, (300, 300, 300), 91, 0.01)
    case = _case()
    net = F.net_on(dev, case.seed, case.latent, case.sd)
    so = case.seg_off.tolist()
    small = (case.pts[so[3]:so[4]], case.tgt[so[3]:so[4]], case.z[3:4], torch.tensor([0, so[4] - so[3]]))
    alone = F.run(net, dev, *small, cutoff=F.CUTOFF, sigma=0.01)
    with poisoned() as p:
        F.run(net, dev, big.pts, big.tgt, case.z[:3], big.seg_off, cutoff=F.CUTOFF, sigma=0.01)
        after = F.run(net, dev, *small, cutoff=F.CUTOFF, sigma=0.01)
        p.check_canaries()
    assert torch.equal(after[0], alone[0]) and torch.equal(after[1], alone[1])
    F.run(net, dev, big.pts, big.tgt, case.z[:3], big.seg_off, cutoff=F.CUTOFF, sigma=0.01)
    again = F.run(net, dev, *small, cutoff=F.CUTOFF, sigma=0.01)
    assert torch.equal(again[0], alone[0]) and torch.equal(again[1], alone[1])


def check_fit_under_poison(dev):
    from shapegan_amd.reconstruct import fit_latent_codes
    case = _case()
    net = F.net_on(dev, case.seed, case.latent, case.sd)
    kw = dict(iterations=3, lr=1e-3, points_per_step=40, seed=1)
    plain = fit_latent_codes(net, case.pts.to(dev), case.tgt.to(dev), case.seg_off.to(dev), **kw)
    with poisoned() as p:
        codes, loss = fit_latent_codes(net, case.pts.to(dev), case.tgt.to(dev), case.seg_off.to(dev), **kw)
        p.check_canaries()
    assert torch.equal(codes.cpu(), plain[0].cpu()) and torch.equal(loss.cpu(), plain[1].cpu())
