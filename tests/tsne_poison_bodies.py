"""Poison-tier bodies of exact t-SNE (tests/poison.py): sg_tsne_affinities writes P in full, diagonal included, and beta and plogp;
sg_tsne_gradient / sg_tsne_step write grad and kl; nothing stale is read (the workspaces hold NaN); two runs are bit-identical; a small
call right after a large one equals the small call alone; tsne() under poison equals the plain run."""
import numpy as np
import torch

import tsne_forms as F
from poison import poisoned
from shapegan_amd import ops
from shapegan_amd import traversal as T

SIZES = (33, 257, 300)      # scalar and float4 gradient paths, a ragged last tile of every kernel


def snapshot(dev, n):
    x = F.t(F.points(n, 3), dev)
    P, beta, plogp = ops.tsne_affinities(x, F.perplexity_for(n))
    y = F.t(F.embedding(n, 3.0), dev)
    grad, kl = ops.tsne_gradient(y, P, 12.0, plogp)
    alone = ops.tsne_gradient(y, P, 12.0)
    vel, gains = torch.zeros_like(y), torch.ones_like(y)
    sgrad, skl = ops.tsne_step(y, P, vel, gains, 1.0, 0.8, 50.0, plogp=plogp)
    return [v.clone() for v in (P, beta, plogp, grad, kl, alone, sgrad, skl, y, vel, gains)]


def check_outputs_and_repeat(dev, n):
    plain = snapshot(dev, n)
    with poisoned() as p:
        first = snapshot(dev, n)
        p.renew()
        second = snapshot(dev, n)
        p.check_canaries()
    for got in (first, second):
        for a, b in zip(got, plain):
            assert not torch.isnan(a).any(), "an output element was not written"
            assert torch.equal(a, b)


def check_small_after_large(dev):
    """The large call's scratch lies where the small call's will: the small call must not see it."""
    alone = snapshot(dev, 33)
    with poisoned() as p:
        snapshot(dev, 300)
        after = snapshot(dev, 33)
        p.check_canaries()
    assert all(torch.equal(a, b) for a, b in zip(after, alone))
    snapshot(dev, 300)
    again = snapshot(dev, 33)
    assert all(torch.equal(a, b) for a, b in zip(again, alone))


def check_tsne_under_poison(dev):
    x = F.t(F.points(65, 3), dev)
    y0 = torch.from_numpy(F.embedding(65, 1e-4))
    kw = dict(perplexity=10, iterations=6, exaggeration_iterations=3, init=y0, return_kl=True)
    plain = T.tsne(x, **kw)
    with poisoned() as p:
        y, kl = T.tsne(x, **kw)
        p.check_canaries()
    assert torch.equal(y, plain[0]) and kl == plain[1] and np.isfinite(kl)
