"""Inputs, float64 references and test bodies of the level-set projection: SDFNet.sdf_and_gradient / project_to_level_set
(csrc/sdfnet_project.hip and its twin) and shapegan_amd/surface.py.  Run on the twin by tests/test_project.py and on the GPU by
tests/test_gpu_project.py; nothing here is a test by itself.

Reference.  oracle.torch_oracle.sdfnet_forward on float64 copies of the state and the inputs with autograd with respect to the points,
and the update rule of include/shapegan_hip.h (K7d) written out in torch; the whole iteration runs once in float64 and once in float32.
Criterion.  sdfnet_forms.check:  |got - ref64| <= 1e-4 * mean|ref64| + 4 * max|ref32 - ref64|, separately for points, value and grad.
Inputs.  Chosen by the float64 reference alone: per shape 60 n candidates uniform in [-1, 1]^3, of which the first n are kept whose
float64 |f - level| < 0.05 and which are safe at every iterate: min |pre-activation| >= 1e-6 (no ReLU kink), the unclipped step length
at least 1e-3 max_step away from max_step (the kink of the clip), |grad f| >= 1e-3.  That enough remain, and that at most 5 % of the
in-band candidates were dropped as unsafe, is asserted.  A seeded network with torch's default initialisation (uniform, variance 1 / (3 fan_in)) is nearly
flat over the cube and its hidden pre-activations shrink with depth, so that a tenth of all points sit on a ReLU kink somewhere along
three steps.  The seeded states here multiply every hidden layer's weight by sqrt(6) — He's variance 2 / fan_in, under which
activations keep their scale through the layers as they do in the trained network — and set the last bias so that the float64 value at
the origin is 0 for the zero code: a level set with |grad f| around 0.1 in the cube, and 1 - 5 % of unsafe candidates."""
import functools

import numpy as np
import pytest
import torch

from latent_fit_forms import Case, chairs_state, net_on, state_of
from oracle import torch_oracle as O
from sdfnet_forms import _Recorder, check, segment_table

BAND = 0.05
MAX_STEP = 0.1
POSITION_RUNS = (1, 31, 32, 33, 63, 64, 65, 129, 2)
RULES = ("newton", "unit")
UNSAFE_SHARE = 0.05


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def value_and_grad(P, x, zrows):
    """f and grad f with respect to the points, in the dtype of P."""
    x = x.clone().requires_grad_(True)
    out = O.sdfnet_forward(P, x, zrows).reshape(-1)
    (g,) = torch.autograd.grad(out.sum(), x)
    return out.detach(), g.detach()


def step(x, out, g, level, rule, max_step):
    """The update rule of the header, in the dtype of x: (x after the step, the unclipped step length)."""
    d = out - level
    n2 = g[:, 0] * g[:, 0] + (g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    nrm = n2.sqrt()
    t = d / n2 if rule == "newton" else d / nrm
    s = t.unsqueeze(1) * g
    length = t.abs() * nrm
    if max_step > 0:
        c = torch.where(length > max_step, max_step / length, torch.ones_like(length))
        s = s * c.unsqueeze(1)
    bad = ~(n2 > 0) | ~torch.isfinite(s).all(dim=1)
    s = torch.where(bad.unsqueeze(1), torch.zeros_like(s), s)
    return x - s, length


def iterate(sd, pts, zrows, level, iterations, rule, max_step, dtype):
    """[(x, f, g)] after 0 .. iterations steps in `dtype`, and the per-point safety of the whole run (meaningful in float64)."""
    P = {k: v.to(dtype) for k, v in sd.items()}
    x, zr = pts.to(dtype), zrows.to(dtype)
    states, safe = [], torch.ones(pts.shape[0], dtype=torch.bool)
    for it in range(iterations + 1):
        f, g = value_and_grad(P, x, zr)
        states.append((x, f, g))
        safe &= O.sdfnet_min_preactivation(P, x, zr) >= 1e-6
        safe &= g.norm(dim=1) >= 1e-3
        if it < iterations:
            x, length = step(x, f, g, level, rule, max_step)
            if max_step > 0:
                safe &= (length - max_step).abs() >= 1e-3 * max_step
    return states, safe


HIDDEN_GAIN = 6 ** 0.5


def weights_of(weights, seed, latent):
    """The chairs state, or a seeded one with a surface in the cube (module docstring)."""
    if weights == "chairs":
        return chairs_state()
    sd = state_of(net_on("cpu", seed, latent))
    for k in sd:
        if k.endswith("weight"):
            sd[k] = sd[k] * (1.0 if k == "layers2.6.weight" else HIDDEN_GAIN)
    sd["layers2.6.bias"] = torch.zeros_like(sd["layers2.6.bias"])
    P64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        centre = O.sdfnet_forward(P64, torch.zeros(1, 3, dtype=torch.float64), torch.zeros(1, latent, dtype=torch.float64)).reshape(-1)
    sd["layers2.6.bias"] = -torch.atanh(centre).float().reshape(1)
    return sd


def codes_of(weights, nshapes, latent, seed):
    return torch.randn(nshapes, latent, generator=torch.Generator().manual_seed(seed + 1)) * 0.1


def safe_points(sd, z, runs, seed, level, iterations, rule, max_step):
    """(points [N,3], seg_off): module docstring."""
    g = torch.Generator().manual_seed(seed)
    P64 = {k: v.double() for k, v in sd.items()}
    pts, dropped, inband = [], 0, 0
    for s, n in enumerate(runs):
        cand = torch.rand(60 * n + 64, 3, generator=g) * 2 - 1
        zs = z[s:s + 1].expand(cand.shape[0], -1)
        with torch.no_grad():
            f = O.sdfnet_forward(P64, cand.double(), zs.double()).reshape(-1)
        band = ((f - level).abs() < BAND).nonzero().flatten()[:2 * n + 8]
        _, safe = iterate(sd, cand[band], zs[band], level, iterations, rule, max_step, torch.float64)
        keep = band[safe][:n]
        assert keep.numel() == n, "shape %d: %d of %d in-band candidates are safe, %d needed" % (s, int(safe.sum()), band.numel(), n)
        dropped += int((~safe).sum())
        inband += band.numel()
        pts.append(cand[keep])
    assert dropped <= UNSAFE_SHARE * inband, "%d of %d in-band candidates were dropped as unsafe" % (dropped, inband)
    return torch.cat(pts), segment_table(list(runs))[1]


@functools.lru_cache(maxsize=None)
def make_case(weights, latent, runs, seed, level, iterations, rule, max_step):
    """Inputs and both reference runs: made once per key, shared, never written."""
    sd = weights_of(weights, seed, latent)
    z = codes_of(weights, len(runs), latent, seed)
    pts, seg_off = safe_points(sd, z, runs, seed + 2, level, iterations, rule, max_step)
    zrows = z[segment_table(list(runs))[0]]
    r32, _ = iterate(sd, pts, zrows, level, iterations, rule, max_step, torch.float32)
    r64, _ = iterate(sd, pts, zrows, level, iterations, rule, max_step, torch.float64)
    return Case(sd=sd, seed=seed, latent=latent, runs=list(runs), z=z, zrows=zrows, pts=pts, seg_off=seg_off, level=level, rule=rule,
                max_step=max_step, r32=r32, r64=r64)


def run(net, dev, pts, z, seg_off, iterations, level=0.0, rule="newton", max_step=MAX_STEP):
    """(points, value, grad) on the CPU after `iterations` steps on `dev`."""
    p, zz, so = pts.to(dev), z.to(dev), None if seg_off is None else seg_off.to(dev)
    if iterations == 0:
        sdf, grad = net.sdf_and_gradient(p, zz, so)
        x = p
    else:
        x, sdf, grad = net.project_to_level_set(p, zz, so, level=level, iterations=iterations, rule=rule, max_step=max_step)
    assert sdf.device.type == torch.device(dev).type and grad.device.type == torch.device(dev).type
    return x.cpu(), sdf.cpu(), grad.cpu()


def check_case(body, dev, case, iterations):
    net = net_on(dev, case.seed, case.latent, case.sd)
    x, f, g = run(net, dev, case.pts, case.z, case.seg_off, iterations, case.level, case.rule, case.max_step)
    what = "%d iterations" % iterations
    for got, k, name in ((x, 0, "points"), (f, 1, "value"), (g, 2, "grad")):
        check(body, got, case.r32[iterations][k], case.r64[iterations][k], "%s after %s" % (name, what))


# ---- bodies -----------------------------------------------------------------------------------------------------------------------
def body_positions(dev, weights, rule, level):
    """Every tile position: runs of 1 .. 129 points in one call, after 0, 1 and 3 steps."""
    case = make_case(weights, 128, POSITION_RUNS, 31, level, 3, rule, MAX_STEP)
    for iterations in (0, 1, 3):
        check_case("positions %s %s level %g" % (weights, rule, level), dev, case, iterations)


def body_latent_sizes(dev, latent):
    check_case("latent size %d" % latent, dev, make_case("seeded", latent, (33, 64, 5), 40 + latent, 0.0, 2, "newton", MAX_STEP), 2)


def _slice(case, order):
    so = case.seg_off.tolist()
    idx = torch.cat([torch.arange(so[s], so[s + 1]) for s in order])
    return case.pts[idx], case.z[list(order)], segment_table([case.runs[s] for s in order])[1]


def _same(a, b, what):
    for x, y, name in zip(a, b, ("points", "value", "grad")):
        assert torch.equal(x, y), "%s: %s differ" % (what, name)


def body_value_is_the_forward(dev):
    """iterations = 0: `value` is point_evaluator's output bit for bit — the forward is the same tile code."""
    case = make_case("seeded", 128, (70, 33, 129), 52, 0.0, 3, "newton", MAX_STEP)
    net = net_on(dev, case.seed, case.latent, case.sd)
    evaluate, _ = net.point_evaluator(case.z.to(dev))
    sid = segment_table(case.runs)[0].int().to(dev)
    expected = evaluate(case.pts.to(dev).contiguous(), sid).cpu()
    _, f, _ = run(net, dev, case.pts, case.z, case.seg_off, 0)
    assert torch.equal(f, expected), "largest difference %g" % float((f - expected).abs().max())


def body_independence(dev, monkeypatch):
    """A shape alone, at each position of a three-shape call, and in chunks: equal bits in all three outputs; a repeat is identical."""
    from shapegan_amd import ops
    case = make_case("seeded", 128, (70, 33, 129), 52, 0.0, 3, "newton", MAX_STEP)
    net = net_on(dev, case.seed, case.latent, case.sd)
    so = case.seg_off.tolist()
    whole = run(net, dev, case.pts, case.z, case.seg_off, 3)
    _same(run(net, dev, case.pts, case.z, case.seg_off, 3), whole, "a repeat")
    for s in range(3):
        alone = run(net, dev, *_slice(case, [s]), 3)
        _same(alone, [t[so[s]:so[s + 1]] for t in whole], "shape %d alone against the whole call" % s)
        others = [t for t in range(3) if t != s]
        for pos in range(3):
            order = others[:pos] + [s] + others[pos:]
            got = run(net, dev, *_slice(case, order), 3)
            first = sum(case.runs[t] for t in order[:pos])
            _same([t[first:first + case.runs[s]] for t in got], alone, "shape %d at position %d" % (s, pos))
    one = run(net, dev, case.pts[:70], case.z[0], None, 3)      # one code [L] owns all points
    _same(one, [t[:70] for t in whole], "a single code without offsets")
    for limit in (1, 2):
        monkeypatch.setattr(ops, "_PROJECT_MAX_SHAPES", limit)
        _same(run(net, dev, case.pts, case.z, case.seg_off, 3), whole, "chunks of %d shapes" % limit)


def body_in_place(dev):
    """out_points aliasing points equals out of place."""
    case = make_case("seeded", 128, (70, 33, 129), 52, 0.0, 3, "newton", MAX_STEP)
    net = net_on(dev, case.seed, case.latent, case.sd)
    whole = run(net, dev, case.pts, case.z, case.seg_off, 3)
    proj = net.surface_projector(case.z.to(dev))
    p = case.pts.to(dev).clone()
    x, f, g = proj.run(p, case.seg_off.numpy(), case.seg_off.to(dev), iterations=3, max_step=MAX_STEP, out_points=p)
    assert x is p
    _same((x.cpu(), f.cpu(), g.cpu()), whole, "in place")


def body_clipped_steps(dev):
    """max_step far below the band's Newton step: a known share of the float64 steps is clipped to it; max_step = 0 never clips."""
    small = 0.01
    case = make_case("chairs", 128, (65, 40), 61, 0.0, 1, "newton", small)
    d64 = (case.r64[1][0] - case.r64[0][0]).norm(dim=1)
    _, length = step(case.r64[0][0], case.r64[0][1], case.r64[0][2], 0.0, "newton", small)
    clipped = length > small
    share = float(clipped.double().mean())
    assert 0.2 <= share <= 0.98, "the case should clip a good share of the steps and leave some: %.3f" % share
    assert float((d64[clipped] - small).abs().max()) < 1e-12
    check_case("clipped steps", dev, case, 1)
    net = net_on(dev, case.seed, case.latent, case.sd)
    x, _, _ = run(net, dev, case.pts, case.z, case.seg_off, 1, max_step=small)
    moved = (x.double() - case.pts.double()).norm(dim=1)
    assert float((moved[clipped] - small).abs().max()) <= 1e-5 * small + 4e-7, "clipped steps are not max_step long"
    assert bool((moved[~clipped] < small).all())
    free = make_case("chairs", 128, (65, 40), 61, 0.0, 1, "newton", 0.0)
    assert float((free.r64[1][0] - free.r64[0][0]).norm(dim=1).max()) > 5 * small, "the unclipped case should take long steps"
    check_case("unclipped steps", dev, free, 1)


def body_zero_gradient(dev):
    """A network whose last layer's weight is zero is constant: grad == 0, every point stays where it is, under both rules."""
    sd = state_of(net_on("cpu", 77, 16))
    sd["layers2.6.weight"] = torch.zeros_like(sd["layers2.6.weight"])
    net = net_on(dev, 77, 16, sd)
    g = torch.Generator().manual_seed(78)
    pts, z = torch.rand(45, 3, generator=g) * 2 - 1, torch.randn(1, 16, generator=g)
    const = float(torch.tanh(sd["layers2.6.bias"].double()))
    assert abs(const) > 1e-3, "the constant should be off the level"
    for rule in RULES:
        x, f, grad = run(net, dev, pts, z, None, 2, rule=rule)
        assert torch.equal(x, pts), "a point moved without a gradient (%s)" % rule
        assert torch.equal(grad, torch.zeros_like(grad))
        assert float((f.double() - const).abs().max()) < 1e-6


def body_no_side_effects(dev):
    """No parameter or point receives a .grad, `points` is unchanged, with grad mode on and off."""
    case = make_case("seeded", 128, (70, 33, 129), 52, 0.0, 3, "newton", MAX_STEP)
    net = net_on(dev, case.seed, case.latent, case.sd)
    results = []
    for no_grad in (False, True):
        p, z, so = case.pts.to(dev).clone(), case.z.to(dev), case.seg_off.to(dev)
        with torch.set_grad_enabled(not no_grad):
            sdf, grad = net.sdf_and_gradient(p, z, so)
            x, f, g = net.project_to_level_set(p, z, so, iterations=2)
        assert torch.equal(p.cpu(), case.pts) and p.grad is None and not p.requires_grad
        assert x.data_ptr() != p.data_ptr()
        for t in (sdf, grad, x, f, g):
            assert not t.requires_grad and t.grad_fn is None
        for q in net.parameters():
            assert q.grad is None, "a parameter received a .grad"
        results.append([t.cpu() for t in (sdf, grad, x, f, g)])
    for a, b in zip(*results):
        assert torch.equal(a, b)


def body_refusals(dev, monkeypatch):
    """Every argument error raises before a launch: the shell's, counted on the library object, and the entry point's own."""
    from shapegan_amd import ops
    case = make_case("seeded", 128, (70, 33, 129), 52, 0.0, 3, "newton", MAX_STEP)
    net = net_on(dev, case.seed, case.latent, case.sd)
    p, z, so = case.pts.to(dev), case.z.to(dev), case.seg_off.to(dev)
    proj = net.surface_projector(z)
    rec = _Recorder(ops._lib())
    monkeypatch.setattr(ops, "_lib", lambda: rec)
    for kw, match in ((dict(iterations=-1), "iterations"), (dict(iterations=65), "iterations"), (dict(rule="secant"), "rule"),
                      (dict(max_step=-0.5), "max_step"), (dict(max_step=float("nan")), "max_step")):
        with pytest.raises(ValueError, match=match):
            net.project_to_level_set(p, z, so, **kw)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        net.sdf_and_gradient(p[:, :2], z, so)
    with pytest.raises(ValueError, match="rows"):
        net.sdf_and_gradient(p, z[:-1], so)
    with pytest.raises(ValueError, match="divide"):
        net.sdf_and_gradient(p[:-2], z, None)
    with pytest.raises(ValueError, match="outside"):
        net.sdf_and_gradient(p[:-1], z, so)
    assert "sg_sdfnet_project" not in rec.calls, "a launch was assembled for a refused argument"
    monkeypatch.undo()
    # the entry point itself: SG_ERR_ARG, and nothing written
    lib = ops._lib()
    tiles = torch.from_numpy(proj._tiles(case.seg_off.numpy(), 0, 3)).to(dev)
    N, T = p.shape[0], tiles.shape[0]
    out = torch.full((N, 3), 7.0, device=dev)
    val, grad = torch.full((N,), 7.0, device=dev), torch.full((N, 3), 7.0, device=dev)
    ptr = ops.ptr
    good = dict(points=p, seg=so, S=3, zb1=proj.zb1, zb5=proj.zb5, packed=proj.packed, level=0.0, it=1, rule=0, step=0.1, tiles=tiles,
                T=T, out=out, val=val, grad=grad)

    def call(**change):
        a = dict(good, **change)
        rc = lib.sg_sdfnet_project(ptr(a["points"]), ptr(a["seg"]), a["S"], ptr(a["zb1"]), ptr(a["zb5"]), ptr(a["packed"]), a["level"],
                                   a["it"], a["rule"], a["step"], ptr(a["tiles"]), a["T"], ptr(a["out"]), ptr(a["val"]), ptr(a["grad"]),
                                   ops.stream())
        ops.L.reset_call_state()
        return rc
    bad = [dict(S=0), dict(T=0), dict(T=1 << 31), dict(it=-1), dict(it=65), dict(rule=2), dict(rule=-1), dict(step=-1.0), dict(out=None)]
    bad += [{k: None} for k in ("seg", "zb1", "zb5", "packed", "tiles", "val", "grad")]
    for change in bad:
        assert call(**change) == -1, "%s was not refused (SG_ERR_ARG)" % (change,)
    if dev != "cpu":
        torch.cuda.synchronize()
    for t in (out, val, grad):
        assert bool((t == 7.0).all()), "a refused call wrote to an output"
    assert call(it=0, out=None) == 0, "out_points may be NULL with iterations == 0"
    assert call() == 0


def body_convergence(dev):
    """Chairs weights, 400 in-band points, Newton, 5 steps: the share of points whose float64 |f| at the returned position is
    at most 1e-4 is no more than one percent below the float64 reference's own share."""
    case = make_case("chairs", 128, (400,), 91, 0.0, 5, "newton", MAX_STEP)
    net = net_on(dev, case.seed, case.latent, case.sd)
    x, _, _ = run(net, dev, case.pts, case.z, case.seg_off, 5)
    P64 = {k: v.double() for k, v in case.sd.items()}
    with torch.no_grad():
        f_got = O.sdfnet_forward(P64, x.double(), case.zrows.double()).reshape(-1)
    share_got = float((f_got.abs() <= 1e-4).double().mean())
    share_ref = float((case.r64[5][1].abs() <= 1e-4).double().mean())
    print("[project] convergence | share within 1e-4: got %.4f, float64 reference %.4f | p99 |f| %.3g" % (
        share_got, share_ref, float(f_got.abs().kthvalue(396).values)))
    assert share_ref > 0.5, "the float64 iteration itself should converge: %.3f" % share_ref
    assert share_got >= share_ref - 0.01


# ---- surface.py: refined meshes, oriented clouds, the renderer's fused normals -------------------------------------------------------
MESH_R = 16
MESH_ITERATIONS = 3
TOLERANCE = 1e-4


def chairs_net(dev):
    sd = chairs_state()
    return net_on(dev, 5, sd["layers1.0.weight"].shape[1] - 3, sd), sd


def mesh_codes():
    return torch.randn(2, 128, generator=torch.Generator().manual_seed(17)) * 0.1


def _unit(g):
    return g / g.norm(dim=1, keepdim=True)


def _restate(sd, start, zrows, level, iterations, max_step):
    """(x, f, unit normal) after the Newton iteration from `start` in float32 and in float64."""
    out = []
    for dtype in (torch.float32, torch.float64):
        states, _ = iterate(sd, start, zrows, level, iterations, "newton", max_step, dtype)
        x, f, g = states[iterations]
        out.append((x, f, _unit(g)))
    return out


def _f64(sd, x, zrows):
    P64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        return O.sdfnet_forward(P64, x.double(), zrows.double()).reshape(-1)


def body_refine_meshes(dev):
    """Two chairs codes at R = 16: connectivity untouched, moved vertices on the surface within tolerance and max_move, kept-back ones
    bit for bit the input, the mean residual lower, positions and normals those of the float64 restatement."""
    from shapegan_amd.reconstruct import reconstruct_meshes
    from shapegan_amd.surface import cell_diagonal, refine_meshes
    net, sd = chairs_net(dev)
    codes = mesh_codes()
    limit = cell_diagonal(MESH_R)
    batch = reconstruct_meshes(net, codes.to(dev), MESH_R)
    refined, stats = refine_meshes(net, codes.to(dev), batch, iterations=MESH_ITERATIONS, max_move=limit, tolerance=TOLERANCE)
    assert torch.equal(refined.faces, batch.faces) and torch.equal(refined.vert_offsets, batch.vert_offsets)
    assert torch.equal(refined.tri_offsets, batch.tri_offsets)
    v0, n0, v1, n1 = batch.vertices.cpu(), batch.normals.cpu(), refined.vertices.cpu(), refined.normals.cpu()
    vo = batch.vert_offsets.cpu()
    counts = vo[1:] - vo[:-1]
    assert int(counts.min()) > 30, "both codes should give a surface at R = %d: %s" % (MESH_R, counts.tolist())
    zrows = codes[torch.repeat_interleave(torch.arange(2), counts)]
    (x32, f32_, u32), (x64, f64_, u64) = _restate(sd, v0, zrows, 0.0, MESH_ITERATIONS, limit)
    moved64 = (x64 - v0.double()).norm(dim=1)
    keep_ref = (f64_.abs() > TOLERANCE) | (moved64 > limit)
    borderline = ((f64_.abs() - TOLERANCE).abs() <= 1e-6) | ((moved64 - limit).abs() <= 1e-6)
    kept = (v1 == v0).all(dim=1) & (n1 == n0).all(dim=1)
    sure = ~borderline
    assert torch.equal(kept[sure], keep_ref[sure]), "%d vertices kept back, the float64 restatement keeps %d" % (int(kept[sure].sum()), int(keep_ref[sure].sum()))
    print("[project] refine_meshes | %d vertices, %d kept back, %d borderline | stats %s" % (v0.shape[0], int(kept.sum()), int(borderline.sum()), stats))
    assert 0 < int((~kept).sum()), "no vertex moved"
    # kept-back vertices are the input bit for bit: by construction of `kept`, every vertex is either that or moved, and a moved one obeys
    f_got, f_before = _f64(sd, v1, zrows), _f64(sd, v0, zrows)
    went = (v1.double() - v0.double()).norm(dim=1)
    assert float(f_got[~kept].abs().max()) <= TOLERANCE, "a moved vertex is %g off the level" % float(f_got[~kept].abs().max())
    assert float(went[~kept].max()) <= limit
    assert float(f_got.abs().mean()) < float(f_before.abs().mean())
    m = sure & ~keep_ref
    check("refine_meshes", v1[m], x32[m], x64[m], "moved vertices")
    check("refine_meshes", n1[m], u32[m], u64[m], "normals of moved vertices")
    assert float((n1[~kept].norm(dim=1) - 1).abs().max()) < 1e-5
    assert stats["vertices"] == counts.tolist()
    sid = torch.repeat_interleave(torch.arange(2), counts)
    assert stats["kept_back"] == torch.zeros(2, dtype=torch.int64).index_add(0, sid, kept.long()).tolist()
    for s in range(2):
        assert stats["mean_after"][s] < stats["mean_before"][s] and stats["max_after"][s] <= stats["max_before"][s]


class _CaptureRenderer(object):
    """Stands in for MeshRenderer in traversal_frames: keeps the batches it is asked to draw."""
    size, ssaa, model_color = 32, 1, None

    def __init__(self):
        self.batches = []

    def render_meshes(self, batch):
        self.batches.append(batch)
        return []


def body_refine_entry_points(dev, tmp_path):
    """refine = 0 is today's mesh bit for bit; refine = 3 through get_mesh, reconstruct_meshes, traversal_frames and the command line gives
    the vertices of refine_meshes called directly."""
    from shapegan_amd import reconstruct
    from shapegan_amd.surface import cell_diagonal, refine_meshes
    from shapegan_amd.traversal import traversal_frames
    from latent_fit_forms import TETRAHEDRA
    net, sd = chairs_net(dev)
    codes = mesh_codes().to(dev)
    plain = reconstruct.reconstruct_meshes(net, codes, MESH_R)
    direct, _ = refine_meshes(net, codes, plain, iterations=3, max_move=cell_diagonal(MESH_R))
    zero = reconstruct.reconstruct_meshes(net, codes, MESH_R, refine=0)
    assert torch.equal(zero.vertices, plain.vertices) and torch.equal(zero.normals, plain.normals) and torch.equal(zero.faces, plain.faces)
    through = reconstruct.reconstruct_meshes(net, codes, MESH_R, refine=3)
    assert torch.equal(through.vertices, direct.vertices) and torch.equal(through.normals, direct.normals)
    cap = _CaptureRenderer()
    assert list(traversal_frames(net, codes, voxel_resolution=MESH_R, level=0.0, renderer=cap, refine=3)) == []
    got = torch.cat([b.vertices for b in cap.batches])
    assert torch.equal(got, direct.vertices), "traversal_frames(refine=3) draws other vertices"
    for s in range(2):
        today, same = net.get_mesh(codes[s], voxel_resolution=MESH_R), net.get_mesh(codes[s], voxel_resolution=MESH_R, refine=0)
        assert np.array_equal(today.vertices, same.vertices) and np.array_equal(today.vertex_normals, same.vertex_normals)
        assert np.array_equal(today.vertices, plain.mesh(s).vertices)
        one = net.get_mesh(codes[s], voxel_resolution=MESH_R, refine=3)
        assert np.array_equal(one.vertices, direct.mesh(s).vertices) and np.array_equal(one.vertex_normals, direct.mesh(s).vertex_normals)
        assert np.array_equal(one.faces, today.faces)
    # the command line (on the CPU, as latent_fit_forms.body_cli): the file it writes is write_obj of reconstruct_meshes(refine=3)
    models = tmp_path / "models" / "abc" / "models"
    models.mkdir(parents=True)
    (models / "model_normalized.obj").write_text(TETRAHEDRA)
    torch.save(sd, str(tmp_path / "sdf_net.to"))
    out = tmp_path / "out" / "codes.to"
    argv = ["--net", str(tmp_path / "sdf_net.to"), "--models", str(tmp_path / "models"), "--out", str(out), "--device", "cpu", "--points", "300",
            "--iterations", "2", "--scan-count", "6", "--scan-resolution", "64", "--resolution", str(MESH_R)]
    assert reconstruct.main(argv + ["--meshes", str(tmp_path / "refined"), "--refine", "3"]) == 0
    assert reconstruct.main(argv + ["--meshes", str(tmp_path / "plain")]) == 0
    fitted = torch.load(str(out))
    cpu_net, _ = chairs_net("cpu")
    expected = reconstruct.reconstruct_meshes(cpu_net, fitted, MESH_R, refine=3)
    reconstruct.write_obj(str(tmp_path / "expected.obj"), expected.mesh(0))
    text = (tmp_path / "refined" / "0000.obj").read_text()
    assert text == (tmp_path / "expected.obj").read_text()
    assert text != (tmp_path / "plain" / "0000.obj").read_text(), "--refine changed nothing"


CLOUD_LEVEL = -0.08
CLOUD_R = 16
CLOUD_COUNT = 150


def cloud_codes():
    """Three codes of the chairs network; the grid of the middle one stays above CLOUD_LEVEL everywhere."""
    return torch.stack([-torch.ones(128), torch.randn(128, generator=torch.Generator().manual_seed(3)) * 0.1, 2 * torch.ones(128)])


def body_oriented_clouds(dev):
    from shapegan_amd.mesh import marching_cubes
    from shapegan_amd.surface import cell_diagonal, sample_oriented_clouds
    net, sd = chairs_net(dev)
    codes = cloud_codes()

    def sample(seed):
        g = torch.Generator().manual_seed(seed)
        return sample_oriented_clouds(net, codes.to(dev), CLOUD_COUNT, voxel_resolution=CLOUD_R, level=CLOUD_LEVEL, iterations=5, generator=g)
    pts, nrm, valid = sample(11)
    again = sample(11)
    assert valid.cpu().tolist() == [True, False, True]
    assert pts.shape == (3, CLOUD_COUNT, 3) and nrm.shape == (3, CLOUD_COUNT, 3)
    for a, b in zip((pts, nrm, valid), again):
        assert torch.equal(a, b), "a repeat with the same seed differs"
    pts, nrm = pts.cpu(), nrm.cpu()
    assert torch.equal(pts[1], torch.zeros(CLOUD_COUNT, 3)) and torch.equal(nrm[1], torch.zeros(CLOUD_COUNT, 3))
    # the restatement: the same start points (grid -> marching cubes -> area-uniform samples), the iteration in torch
    grids = net.voxel_grids(codes.to(dev), CLOUD_R, sphere_only=True, level=CLOUD_LEVEL)
    batch = marching_cubes(grids, level=CLOUD_LEVEL, spacing=2.0 / CLOUD_R, origin=-1.0, pad=True, pad_value=1.0)
    start = batch.sample_surface(CLOUD_COUNT, generator=torch.Generator().manual_seed(11)).cpu()
    live = [0, 2]
    zrows = codes[live].repeat_interleave(CLOUD_COUNT, dim=0)
    (x32, _, u32), (x64, f64_, u64) = _restate(sd, start[live].reshape(-1, 3), zrows, CLOUD_LEVEL, 5, cell_diagonal(CLOUD_R))
    check("oriented clouds", pts[live].reshape(-1, 3), x32, x64, "points")
    check("oriented clouds", nrm[live].reshape(-1, 3), u32, u64, "normals")
    assert float((nrm[live].reshape(-1, 3).norm(dim=1) - 1).abs().max()) < 1e-5
    before = (_f64(sd, start[live].reshape(-1, 3), zrows) - CLOUD_LEVEL).abs().mean()
    after = (_f64(sd, pts[live].reshape(-1, 3), zrows) - CLOUD_LEVEL).abs().mean()
    print("[project] oriented clouds | mean |f - level| %.3g at the samples, %.3g after the projection" % (float(before), float(after)))
    assert float(after) < float(before)


RENDER_SETTINGS = dict(radius=1.6, sdf_offset=-0.045, vertical_cutoff=1)      # those of the stored images (tests/test_gpu_render.py)


def _images_close(a, b):
    """The criterion of test_gpu_render.test_gpu_matches_reference: at most 1 % of the pixels more than 8 apart, mean difference <= 1.5."""
    d = np.abs(np.asarray(a).astype(np.int32) - np.asarray(b).astype(np.int32))
    print("[project] render | share of pixels more than 8 apart %.4f, mean difference %.3f" % ((d.max(axis=-1) > 8).mean(), d.mean()))
    assert (d.max(axis=-1) > 8).mean() <= 0.01 and d.mean() <= 1.5, ((d.max(axis=-1) > 8).mean(), d.mean())


def body_fused_render(dev):
    """32 px, ssaa 1, a chairs code: normals="fused" gives the "autograd" image within the raymarch golden test's own tolerance; the
    default is the "autograd" path bit for bit, and still the stored image of tests/golden/raymarch_chairs.npz under that tolerance."""
    import os
    from latent_fit_forms import GOLDEN
    from shapegan_amd.rendering import raymarching
    net, _ = chairs_net(dev)
    gold = np.load(os.path.join(GOLDEN, "raymarch_chairs.npz"))
    code = torch.from_numpy(gold["latents"][0]).to(dev)
    kw = dict(resolution=32, ssaa=1, **RENDER_SETTINGS)
    default = raymarching.render_image(net, code, **kw)
    auto = raymarching.render_image(net, code, normals="autograd", **kw)
    fused = raymarching.render_image(net, code, normals="fused", **kw)
    assert np.array_equal(np.asarray(default), np.asarray(auto))
    _images_close(default, gold["image_ssaa1_0"])
    _images_close(fused, auto)
    assert np.asarray(fused).std() > 0
    with pytest.raises(ValueError, match="normals"):
        raymarching.render_image(net, code, normals="central", **kw)
