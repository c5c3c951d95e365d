"""Poison-tier bodies of the level-set projection (tests/poison.py): sg_sdfnet_project writes every element of every output row, ragged
last tiles included, and `value` / `grad` alone when out_points is NULL; nothing stale is read; two runs are bit-identical; a small call
right after a large one equals the small call alone."""
import torch

import project_forms as F
from poison import poisoned

RUNS = (1, 31, 33, 65, 200, 2)      # one lane, a tile less one, a tile and one, two tiles and one, seven tiles less 24, two lanes
FORMS = ((0, "newton"), (1, "newton"), (3, "unit"))      # iterations (0: out_points is NULL), rule


def _case():
    return F.make_case("seeded", 29, RUNS, 69, 0.0, 3, "newton", F.MAX_STEP)


def snapshot(dev, iterations, rule):
    case = _case()
    net = F.net_on(dev, case.seed, case.latent, case.sd)
    return [t.clone() for t in F.run(net, dev, case.pts, case.z, case.seg_off, iterations, rule=rule)]


def check_outputs_and_repeat(dev, iterations, rule):
    plain = snapshot(dev, iterations, rule)
    with poisoned() as p:
        first = snapshot(dev, iterations, rule)
        p.renew()
        second = snapshot(dev, iterations, rule)
        p.check_canaries()
    for got in (first, second):
        for t, q in zip(got, plain):
            assert not torch.isnan(t).any(), "an output element was not written"
            assert torch.equal(t, q)


def check_small_after_large(dev):
    """The large call's outputs lie where the small call's will (the allocator hands the blocks back): the small call must not see them."""
    big = F.make_case("seeded", 29, (300, 300, 300), 69, 0.0, 3, "newton", F.MAX_STEP)
    case = _case()
    net = F.net_on(dev, case.seed, case.latent, case.sd)
    so = case.seg_off.tolist()
    small = (case.pts[so[3]:so[4]], case.z[3:4], torch.tensor([0, so[4] - so[3]]))
    alone = F.run(net, dev, *small, 3)
    with poisoned() as p:
        F.run(net, dev, big.pts, big.z, big.seg_off, 3)
        after = F.run(net, dev, *small, 3)
        p.check_canaries()
    F.run(net, dev, big.pts, big.z, big.seg_off, 3)
    again = F.run(net, dev, *small, 3)
    for a, b, c in zip(after, again, alone):
        assert torch.equal(a, c) and torch.equal(b, c)


def check_surface_under_poison(dev):
    """refine_meshes and sample_oriented_clouds under poison equal their plain runs."""
    from shapegan_amd.reconstruct import reconstruct_meshes
    from shapegan_amd.surface import cell_diagonal, refine_meshes, sample_oriented_clouds
    net, _ = F.chairs_net(dev)
    codes = F.mesh_codes().to(dev)

    def both():
        batch = reconstruct_meshes(net, codes, F.MESH_R)
        refined, _ = refine_meshes(net, codes, batch, iterations=2, max_move=cell_diagonal(F.MESH_R))
        cloud = sample_oriented_clouds(net, codes, 40, voxel_resolution=F.MESH_R, generator=torch.Generator().manual_seed(5))
        return [refined.vertices.cpu(), refined.normals.cpu()] + [t.cpu() for t in cloud]
    plain = both()
    with poisoned() as p:
        got = both()
        p.check_canaries()
    for a, b in zip(got, plain):
        assert not torch.isnan(a.float()).any() and torch.equal(a, b)
