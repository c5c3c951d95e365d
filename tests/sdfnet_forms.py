"""Inputs, float64 references, checks and test bodies for the fused SDFNet MLP in every calling form
(tests/test_gpu_sdfnet_forms.py; re-run on the twin by tests/test_cpu_twin.py).  Pure Python: nothing here is a test by itself.

Reference.  oracle.torch_oracle.sdfnet_forward on a float64 copy of the state and the inputs, and again in float32; autograd of
    sum(out * dy) [+ 0.5 * scale * sum_s w_s |z_s|^2 where a latent regulariser is given]
in each precision.  The latents of a point are z[rows[point]] (per-shape forms) or its own row (per-point form).

Criterion.  Gradients: test_gpu_modules.check_against_oracles at its defaults,
    |got - ref64| <= 1e-4 * mean|ref64| + 4 * max|ref32 - ref64|,   at most 0.1 % of the elements (or 4) beyond it, those within
    5 % of the tensor's largest entry.
Forward outputs: rtol 1e-4, atol 2e-6 against float64.  Points whose smallest float64 |pre-activation| is below 1e-6 sit on a ReLU
kink and get no upstream gradient (their share is asserted to stay under 0.1); a point that carries a one-hot upstream gradient is
redrawn from its seed until the reference calls it safe.  Both decisions use the reference alone.  A gradient that was not asked
for must come back None from the autograd Function itself (autograd drops what a Function returns for an input that does not
require grad, so the Function's backward is also called by hand).

Every check prints `[sdfnet-forms] body | what | err/tol | elements beyond tol` before it asserts, and WORST keeps the largest
err / tol per body."""
import functools

import pytest
import torch

import test_gpu_modules as M
import test_gpu_ops as OPS
from oracle import torch_oracle as O

WORST = {}
FRAGILE_BELOW = 1e-6
FRAGILE_CAP = 0.1


# ---- nets, references, checks -------------------------------------------------------------------------------------------------
def make_net(seed, latent):
    """(on the device the bodies run on: OPS.DEV is "cpu" under test_cpu_twin's on_cpu fixture)"""
    from shapegan_amd.model.sdf_net import SDFNet
    torch.manual_seed(seed)
    return SDFNet(latent_code_size=latent, device=OPS.DEV)


def state_of(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def _latents(z, rows):
    return z if rows is None else z[rows]


def fragile_points(sd, pts, z, rows):
    P = {k: v.double() for k, v in sd.items()}
    return O.sdfnet_min_preactivation(P, pts.double(), _latents(z.double(), rows)) < FRAGILE_BELOW


def reference(sd, pts, z, rows, dy, dtype, reg=None):
    """out and the gradients of sum(out * dy) + regulariser in `dtype`: dict(out, points, latents, params{name})."""
    P = O.clone_state({k: v.to(dtype) for k, v in sd.items()})
    p = pts.to(dtype).clone().requires_grad_(True)
    zz = z.to(dtype).clone().requires_grad_(True)
    out = O.sdfnet_forward(P, p, _latents(zz, rows)).reshape(-1)
    scalar = (out * dy.to(dtype)).sum()
    if reg is not None:
        scalar = scalar + regulariser(zz, reg, dtype)
    scalar.backward()
    return dict(out=out.detach(), points=p.grad, latents=zz.grad, params={k: v.grad for k, v in P.items()})


def regulariser(z, reg, dtype):
    """0.5 * scale * sum_s w_s |z_s|^2 (w = 1 without row weights): what latent_reg = (w, scale) is the gradient of."""
    w, scale = reg
    sq = (z * z).sum(dim=1)
    return 0.5 * scale * (sq.sum() if w is None else (sq * w.to(dtype)).sum())


def references(sd, pts, z, rows, dy, reg=None):
    return reference(sd, pts, z, rows, dy, torch.float32, reg), reference(sd, pts, z, rows, dy, torch.float64, reg)


def masked_upstream(sd, pts, z, rows, seed):
    """A random upstream gradient, zero on the points the float64 reference calls fragile."""
    fragile = fragile_points(sd, pts, z, rows)
    share = float(fragile.float().mean())
    assert share < FRAGILE_CAP, "%.3f of the points sit on a ReLU kink" % share
    dy = torch.randn(pts.shape[0], generator=torch.Generator().manual_seed(seed))
    dy[fragile] = 0
    return dy


def _note(body, what, ratio, beyond, numel):
    print("[sdfnet-forms] %s | %s | err/tol %.3g | %d of %d beyond tol" % (body, what, ratio, beyond, numel))
    WORST[body] = max(WORST.get(body, 0.0), ratio)


def check(body, got, ref32, ref64, what):
    """check_against_oracles, behind a printed err / tol of the same formula."""
    assert got is not None, what + ": no gradient came back"
    g, r32, r64 = got.detach().double().cpu(), ref32.detach().double(), ref64.detach().double()
    assert g.shape == r64.shape, "%s: shape %s, reference %s" % (what, tuple(g.shape), tuple(r64.shape))
    tol = M.RTOL * float(r64.abs().mean()) + 4.0 * float((r32 - r64).abs().max())
    err = (g - r64).abs()
    if tol == 0.0:       # the reference is exactly zero in both precisions
        assert float(err.max()) == 0.0, what + ": non-zero where both references are exactly zero"
        _note(body, what, 0.0, 0, g.numel())
        return
    _note(body, what, float(err.max()) / tol, int((err > tol).sum()), g.numel())
    M.check_against_oracles(got, ref32, ref64, what)


def check_forward(body, out, ref64, what):
    got, ref = out.detach().float().cpu().reshape(-1), ref64.float().reshape(-1)
    ratio = float(((got - ref).abs() / (2e-6 + OPS.RTOL * ref.abs())).max())
    _note(body, what + " (forward)", ratio, int(((got - ref).abs() > 2e-6 + OPS.RTOL * ref.abs()).sum()), got.numel())
    OPS.close(got, ref, atol=2e-6, what=what + " forward")


def check_params(body, net, grads, r32, r64, what):
    for (k, _), g in zip(net.named_parameters(), grads):
        check(body, g, r32["params"][k], r64["params"][k], "%s grad %s" % (what, k))


def function_node(out):
    """The autograd node of the fused MLP's own Function behind `out` (net(points, latents) adds a squeeze)."""
    node = out.grad_fn
    while node is not None and not hasattr(node, "_forward_cls"):
        node = node.next_functions[0][0]
    assert node is not None, "no custom Function behind the output"
    return node


def returned_by_backward(out, dy, first_param):
    """What the Function's backward itself returns for (points, latents, the 16 parameters)."""
    raw = function_node(out).apply(dy)
    return raw[1], raw[2], list(raw[first_param:])


def segment_table(runs):
    """(shape index int32 [N], offsets int64 [S + 1]) of consecutive runs of the given lengths."""
    counts = torch.tensor(runs, dtype=torch.int64)
    sid = torch.repeat_interleave(torch.arange(len(runs)), counts)
    seg_off = torch.zeros(len(runs) + 1, dtype=torch.int64)
    seg_off[1:] = torch.cumsum(counts, 0)
    return sid, seg_off


class Case(object):
    """Inputs and references of one case: made once, shared by the bodies that need them, never written."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _net_of(case):
    net = make_net(case.seed, case.latent)
    net.load_state_dict(case.sd)
    return net


def _run(net, case, pts, z, reg=None):
    if case.mode == "points":
        return net(pts, z).reshape(-1)
    if case.mode == "uniform":
        return net.forward_shapes(pts, z, case.pps)
    return net.forward_segments(pts, z, OPS.dev(case.sid.int()), OPS.dev(case.seg_off), reg)


def _make_case(mode, seed, latent, N=None, S=None, pps=None, runs=None, sid=None):
    net = make_net(seed, latent)
    sd = state_of(net)
    g = torch.Generator().manual_seed(seed + 1)
    seg_off = None
    if mode == "points":
        rows, nz = None, N
    elif mode == "uniform":
        N, nz = S * pps, S
        rows = torch.arange(S).repeat_interleave(pps)
    else:
        if runs is not None:
            sid, seg_off = segment_table(runs)
            S = len(runs)
        else:
            seg_off = torch.zeros(S + 1, dtype=torch.int64)
            seg_off[1:] = torch.cumsum(torch.bincount(sid, minlength=S), 0)
        N, nz, rows = sid.shape[0], S, sid
    pts = torch.rand(N, 3, generator=g) * 2 - 1
    z = torch.randn(nz, latent, generator=g) * 0.5
    return Case(mode=mode, seed=seed, latent=latent, N=N, S=S, pps=pps, sd=sd, pts=pts, z=z, rows=rows, sid=sid, seg_off=seg_off)


def _with_references(case, dy_seed):
    case.dy = masked_upstream(case.sd, case.pts, case.z, case.rows, dy_seed)
    case.r32, case.r64 = references(case.sd, case.pts, case.z, case.rows, case.dy)
    return case


def _exact_rows(got, expected, rows, what):
    got, expected = got.detach().cpu(), expected.detach().cpu()
    for s in rows:
        assert torch.equal(got[s], expected[s]), "%s: row %d is %s, expected exactly %s" % (what, s, got[s][:4], expected[s][:4])


def _reg_row(z, reg):
    """row_weight[s] * scale * z[s] in float32, in the order the backward multiplies."""
    w, scale = reg
    return z * scale if w is None else z * (w * scale).unsqueeze(1)


def _reg_grad(z, reg, dtype):
    zz = z.to(dtype).clone().requires_grad_(True)
    regulariser(zz, reg, dtype).backward()
    return zz.grad


# ---- A: which inputs require grad ------------------------------------------------------------------------------------------
MODES = ("points", "uniform", "ragged")
SUBSETS = [(p, z, w) for p in (True, False) for z in (True, False) for w in (True, False) if p or z or w]


@functools.lru_cache(maxsize=None)
def _case_a(mode):
    if mode == "points":
        case = _make_case(mode, 21, 32, N=200)                     # three 64-point tiles and 8 points of a fourth
    elif mode == "uniform":
        case = _make_case(mode, 22, 32, S=3, pps=128)
    else:
        case = _make_case(mode, 23, 32, runs=[70, 0, 101, 64, 65])   # 300 points: the last tile holds 44
    return _with_references(case, 5)


def body_which_grads(mode, need_p, need_z, need_w):
    body = "A which-grads"
    case = _case_a(mode)
    what = "%s p%d z%d w%d" % (mode, need_p, need_z, need_w)
    net = _net_of(case)
    for p in net.parameters():
        p.requires_grad_(need_w)
    pts, z = OPS.dev(case.pts).requires_grad_(need_p), OPS.dev(case.z).requires_grad_(need_z)
    out = _run(net, case, pts, z)
    check_forward(body, out, case.r64["out"], what)
    dy = OPS.dev(case.dy)
    gp, gz, gw = returned_by_backward(out, dy, 4 if mode == "points" else 8)
    assert (gp is not None) == need_p, what + ": d points " + ("missing" if need_p else "returned although not asked for")
    assert (gz is not None) == need_z, what + ": d latents " + ("missing" if need_z else "returned although not asked for")
    assert all((g is not None) == need_w for g in gw), what + ": the parameter gradients are not all " + ("there" if need_w else "None")
    asked = ([pts] if need_p else []) + ([z] if need_z else []) + (list(net.parameters()) if need_w else [])
    grads = list(torch.autograd.grad(out, asked, dy))
    if need_p:
        check(body, grads.pop(0), case.r32["points"], case.r64["points"], what + " d points")
    if need_z:
        check(body, grads.pop(0), case.r32["latents"], case.r64["latents"], what + " d latents")
    if need_w:
        check_params(body, net, grads, case.r32, case.r64, what)


# ---- B: ragged segments by position -------------------------------------------------------------------------------------------
POSITION_RUNS = [64, 0, 1, 63, 65, 126, 127, 128, 129, 0, 0, 192, 31, 32, 33]
POSITION_N = 16384 + 16 * 64 + 40       # the backward's plan: 256 tiles of 64 points, then 34 of 32
POSITION_NBIG = 256


def position_runs():
    """POSITION_RUNS from point 0; one run up to 20 points short of nbig * 64; a run of 50 across nbig * 64; the short runs again
    inside the 32-point tiles, starting off a tile boundary (30 points in), on one (after 2 more points) and wherever they fall;
    a last run up to POSITION_N."""
    edge = POSITION_NBIG * 64
    runs = list(POSITION_RUNS)
    runs.append(edge - 20 - sum(runs))
    runs.append(50)
    runs += [0, 1, 1, 64, 0, 1, 63, 65, 126, 127, 128, 0, 31, 32, 33]
    runs.append(POSITION_N - sum(runs))
    assert runs[-1] > 0
    return runs


def check_position_plan():
    """The tile plan the run lengths were placed for (host code of the HIP library: no device needed)."""
    import shapegan_amd.lib as L
    lib = L.load()
    assert lib.sg_sdfnet_bwd_blocks(POSITION_N) == POSITION_NBIG + 34
    assert lib.sg_sdfnet_bwd_tile_start(POSITION_N, POSITION_NBIG) == POSITION_NBIG * 64
    assert lib.sg_sdfnet_bwd_tile_start(POSITION_N, POSITION_NBIG + 1) == POSITION_NBIG * 64 + 32
    _, seg_off = segment_table(position_runs())
    edge = POSITION_NBIG * 64
    assert any(int(a) < edge < int(b) for a, b in zip(seg_off[:-1], seg_off[1:])), "no run straddles nbig * 64"
    assert int(seg_off[-1]) == POSITION_N


@functools.lru_cache(maxsize=None)
def _case_b():
    case = _make_case("ragged", 31, 16, runs=position_runs())
    case.weights = torch.rand(case.S, generator=torch.Generator().manual_seed(32)) + 0.5
    case.scale = 0.01
    return _with_references(case, 6)


def _empty_rows(case):
    return [s for s in range(case.S) if int(case.seg_off[s + 1]) == int(case.seg_off[s])]


def body_segments_dense(with_reg):
    """with_reg: every gradient asked for, latent_reg = (weights, scale).  Without: the latent table alone requires grad (the
    finishing launch then has no bias gradients to make)."""
    body = "B positions"
    check_position_plan()
    case = _case_b()
    what = "positions " + ("all grads, reg" if with_reg else "table only")
    net = _net_of(case)
    for p in net.parameters():
        p.requires_grad_(with_reg)
    pts, z = OPS.dev(case.pts).requires_grad_(with_reg), OPS.dev(case.z).requires_grad_(True)
    reg = (OPS.dev(case.weights), case.scale) if with_reg else None
    out = _run(net, case, pts, z, reg)
    check_forward(body, out, case.r64["out"], what)
    asked = [z] + ([pts] + list(net.parameters()) if with_reg else [])
    grads = list(torch.autograd.grad(out, asked, OPS.dev(case.dy)))
    gz = grads.pop(0)
    r32, r64 = case.r32["latents"], case.r64["latents"]
    expected = torch.zeros_like(case.z)
    if with_reg:
        cpu_reg = (case.weights, case.scale)
        r32, r64 = r32 + _reg_grad(case.z, cpu_reg, torch.float32), r64 + _reg_grad(case.z, cpu_reg, torch.float64)
        expected = _reg_row(case.z, cpu_reg)
    empty = _empty_rows(case)
    assert len(empty) >= 6
    _exact_rows(gz, expected, empty, what + " d table, empty shape")
    for s in range(case.S):       # row by row: a wrong short run must not hide behind the long ones
        check(body, gz[s], r32[s], r64[s], what + " d table row %d (%d points from %d)" % (
            s, int(case.seg_off[s + 1] - case.seg_off[s]), int(case.seg_off[s])))
    check(body, gz, r32, r64, what + " d table")
    if with_reg:
        check(body, grads.pop(0), case.r32["points"], case.r64["points"], what + " d points")
        check_params(body, net, grads, case.r32, case.r64, what)


ONE_HOT_POSITIONS = {"tile_start": 5 * 64, "last_big": POSITION_NBIG * 64 - 1, "first_small": POSITION_NBIG * 64, "last": POSITION_N - 1}


def body_segments_one_hot(where):
    """Upstream gradient 1 on one point: its shape's table row and its own point gradient against the reference of that point
    alone; every other row of both is exactly zero."""
    body = "B positions"
    case = _case_b()
    i = ONE_HOT_POSITIONS[where]
    s = int(case.sid[i])
    g = torch.Generator().manual_seed(7000 + i)
    while True:
        xyz = (torch.rand(1, 3, generator=g) * 2 - 1)
        if not bool(fragile_points(case.sd, xyz, case.z[s:s + 1], None)[0]):
            break
    one = torch.ones(1)
    r32, r64 = references(case.sd, xyz, case.z[s:s + 1], None, one)
    cpu_pts = case.pts.clone()
    cpu_pts[i] = xyz[0]
    dy = torch.zeros(case.N)
    dy[i] = 1.0
    net = _net_of(case)
    for p in net.parameters():
        p.requires_grad_(False)
    pts, z = OPS.dev(cpu_pts).requires_grad_(True), OPS.dev(case.z).requires_grad_(True)
    out = _run(net, case, pts, z)
    gp, gz = torch.autograd.grad(out, [pts, z], OPS.dev(dy))
    what = "one-hot %s (point %d, shape %d)" % (where, i, s)
    check(body, gz[s], r32["latents"][0], r64["latents"][0], what + " d table row")
    check(body, gp[i], r32["points"][0], r64["points"][0], what + " d point")
    _exact_rows(gz, torch.zeros_like(case.z), [r for r in range(case.S) if r != s], what + " d table, other shape")
    others = torch.ones(case.N, dtype=torch.bool)
    others[i] = False
    assert not bool(gp.detach().cpu()[others].ne(0).any()), what + ": a point without upstream gradient has a gradient"


DEGENERATE = {"one_shape": [200], "all_in_last": [0, 0, 0, 200], "ends_empty": [0, 137, 63, 0]}


@functools.lru_cache(maxsize=None)
def _case_degenerate(kind):
    case = _make_case("ragged", 33, 16, runs=DEGENERATE[kind])
    case.weights = torch.rand(case.S, generator=torch.Generator().manual_seed(34)) + 0.5
    case.scale = 0.01
    return _with_references(case, 7)


def body_segments_degenerate(kind):
    body = "B positions"
    case = _case_degenerate(kind)
    net = _net_of(case)
    pts, z = OPS.dev(case.pts).requires_grad_(True), OPS.dev(case.z).requires_grad_(True)
    out = _run(net, case, pts, z, (OPS.dev(case.weights), case.scale))
    check_forward(body, out, case.r64["out"], kind)
    grads = list(torch.autograd.grad(out, [pts, z] + list(net.parameters()), OPS.dev(case.dy)))
    cpu_reg = (case.weights, case.scale)
    check(body, grads.pop(0), case.r32["points"], case.r64["points"], kind + " d points")
    gz = grads.pop(0)
    _exact_rows(gz, _reg_row(case.z, cpu_reg), _empty_rows(case), kind + " d table, empty shape")
    for s in range(case.S):
        check(body, gz[s], (case.r32["latents"] + _reg_grad(case.z, cpu_reg, torch.float32))[s],
              (case.r64["latents"] + _reg_grad(case.z, cpu_reg, torch.float64))[s], kind + " d table row %d" % s)
    check_params(body, net, grads, case.r32, case.r64, kind)


# ---- C: more shapes than the one-launch fold takes -------------------------------------------------------------------------------
REG_STATES = ("none", "scale", "counts")
FOLD_CASES = [(S, reg, z_only) for S in (1024, 1025) for reg in REG_STATES for z_only in (False, True)] + [
    (40, reg, False) for reg in REG_STATES]


@functools.lru_cache(maxsize=None)
def _case_c(S):
    sid = torch.sort(torch.randint(0, S, (3000,), generator=torch.Generator().manual_seed(40 + S)))[0]
    case = _make_case("ragged", 41, 32, S=S, sid=sid)
    case.counts = torch.bincount(sid, minlength=S).float()
    case.scale = 0.01
    return _with_references(case, 8)


def body_beyond_fold(S, reg_state, z_only):
    from shapegan_amd import ops
    assert ops._FOLD_MAX_SHAPES == 1024      # S = 1024 / 1025 stand on the two sides of it
    body = "C beyond the fold"
    case = _case_c(S)
    what = "S %d reg %s %s" % (S, reg_state, "z only" if z_only else "z and parameters")
    cpu_reg = {"none": None, "scale": (None, case.scale), "counts": (case.counts, case.scale)}[reg_state]
    reg = None if cpu_reg is None else (None if cpu_reg[0] is None else OPS.dev(cpu_reg[0]), cpu_reg[1])
    net = _net_of(case)
    for p in net.parameters():
        p.requires_grad_(not z_only)
    pts, z = OPS.dev(case.pts), OPS.dev(case.z).requires_grad_(True)
    out = _run(net, case, pts, z, reg)
    check_forward(body, out, case.r64["out"], what)
    dy = OPS.dev(case.dy)
    gp, gz_raw, gw = returned_by_backward(out, dy, 8)
    assert gp is None and gz_raw is not None and all((g is None) == z_only for g in gw), what + ": which gradients came back"
    grads = list(torch.autograd.grad(out, [z] + ([] if z_only else list(net.parameters())), dy))
    r32, r64 = case.r32["latents"], case.r64["latents"]
    if cpu_reg is not None:       # (the gradient of the sum of two scalars: autograd adds the two contributions the same way)
        r32, r64 = r32 + _reg_grad(case.z, cpu_reg, torch.float32), r64 + _reg_grad(case.z, cpu_reg, torch.float64)
    gz = grads.pop(0)
    check(body, gz, r32, r64, what + " d table")
    empty = _empty_rows(case)
    assert S < 1024 or len(empty) > 0
    _exact_rows(gz, torch.zeros_like(case.z) if cpu_reg is None else _reg_row(case.z, cpu_reg), empty, what + " d table, empty shape")
    if not z_only:
        check_params(body, net, grads, case.r32, case.r64, what)


# ---- D: the three ways the per-shape fold is made ------------------------------------------------------------------------------
class _Recorder(object):
    """Stands in for the library object the shells call: notes the entry points they ask for."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self.lib, name)


def body_fold_forms():
    from shapegan_amd import ops, optim
    body = "D fold forms"
    S, pps, latent = 3, 128, 32
    net = make_net(51, latent)
    opt = optim.Adam(list(net.parameters()), lr=1e-3)      # parameters in a flat buffer: only then a weight image is ever kept
    g = torch.Generator().manual_seed(52)
    cpu_pts, cpu_z = torch.rand(S * pps, 3, generator=g) * 2 - 1, torch.randn(S, latent, generator=g) * 0.5
    pts, z = OPS.dev(cpu_pts), OPS.dev(cpu_z)
    rows = torch.arange(S).repeat_interleave(pps)
    rec = _Recorder(ops._lib())
    real = ops._lib
    ops._lib = lambda: rec
    try:
        with torch.no_grad():
            net.forward_shapes(pts, z, pps)                       # (whatever state the image was in: it is current now)
            net.layers2[0].bias.add_(0.125)                       # a parameter write
            sd = state_of(net)
            outs = []
            for state in ("stale", "current", "prepared"):
                if state == "prepared":
                    net.prepare_latents(z)
                del rec.calls[:]
                outs.append(net.forward_shapes(pts, z, pps))
                folds = [c for c in rec.calls if c in ("sg_sdfnet_pack", "sg_sdfnet_pack_shape_bias", "sg_sdfnet_shape_bias")]
                assert folds == {"stale": ["sg_sdfnet_pack_shape_bias"], "current": ["sg_sdfnet_shape_bias"], "prepared": []}[state], (state, folds)
                assert "sg_sdfnet_fwd" in rec.calls
            assert torch.equal(outs[0], outs[1]), "pack + fold in one launch differs from the fold alone"
            assert torch.equal(outs[0], outs[2]), "the fold made ahead differs from the forward's own"
            net.prepare_latents(z)
            z.mul_(-0.75)                                         # the prepared fold belongs to the old latents now
            del rec.calls[:]
            moved = net.forward_shapes(pts, z, pps)
            assert "sg_sdfnet_shape_bias" in rec.calls, "a fold prepared for other latents was taken"
    finally:
        ops._lib = real
    ref_old = O.sdfnet_forward({k: v.double() for k, v in sd.items()}, cpu_pts.double(), cpu_z.double()[rows])
    ref_new = O.sdfnet_forward({k: v.double() for k, v in sd.items()}, cpu_pts.double(), (cpu_z.double() * -0.75)[rows])
    check_forward(body, outs[0], ref_old, "after a parameter write")
    check_forward(body, moved, ref_new, "latents changed behind prepare_latents")
    del opt


# ---- E: arguments of the C ABI that no shell passes ---------------------------------------------------------------------------
def _raw_points_fwd(lib, packed, pts, period, lat, idx, latent, N, train):
    """sg_sdfnet_fwd in per-point mode -> (out, the seven activation images or None)."""
    from shapegan_amd.lib import check, ptr, stream
    out = torch.zeros(N, dtype=torch.float32, device=pts.device)
    acts = torch.zeros(lib.sg_sdfnet_acts_floats(N), dtype=torch.float32, device=pts.device) if train else None
    check(lib.sg_sdfnet_fwd(ptr(pts), period, ptr(lat), ptr(idx), latent, ptr(packed), 3 + latent, None, None, 0, None, ptr(out),
                            ptr(acts), N, N, stream()), "sdfnet_fwd")
    return out, (acts[:7 * 256 * N] if train else None)


def body_raw_abi(train):
    import ctypes
    import shapegan_amd.lib as L
    from shapegan_amd.lib import check, f32c, ptr, stream
    body = "E raw ABI"
    lib = L.load()
    latent, period = 32, 94
    N = 3 * period + 17
    net = make_net(61, latent)
    sd = state_of(net)
    params = [f32c(p.detach()) for p in net._params()]
    packed = torch.empty(lib.sg_sdfnet_packed_floats(3 + latent), dtype=torch.float32, device=params[0].device)
    arr = (ctypes.c_void_p * 16)(*[ptr(p) for p in params])
    check(lib.sg_sdfnet_pack(arr, latent, 3 + latent, ptr(packed), stream()), "sdfnet_pack")
    g = torch.Generator().manual_seed(62)
    cpu_pts, cpu_table = torch.rand(N, 3, generator=g) * 2 - 1, torch.randn(7, latent, generator=g) * 0.5
    cpu_idx = torch.randint(0, 7, (N,), generator=g)          # repeated rows, in no order
    cpu_idx[:4] = torch.tensor([6, 6, 0, 3])
    pts, table, idx = OPS.dev(cpu_pts), OPS.dev(cpu_table), OPS.dev(cpu_idx)
    assert idx.dtype == torch.int64
    rows = OPS.dev(cpu_table[cpu_idx].contiguous())
    a = _raw_points_fwd(lib, packed, pts, 0, table, idx, latent, N, train)
    b = _raw_points_fwd(lib, packed, pts, 0, rows, None, latent, N, train)
    assert torch.equal(a[0], b[0]), "latent = table + latent_idx differs from the gathered rows"
    assert not train or torch.equal(a[1], b[1]), "latent_idx: the activation images differ"
    check_forward(body, b[0], O.sdfnet_forward({k: v.double() for k, v in sd.items()}, cpu_pts.double(), cpu_table.double()[cpu_idx]),
                  "gathered rows, train %d" % train)
    grid = OPS.dev(cpu_pts[:period].contiguous())
    tiled = OPS.dev(cpu_pts[:period][torch.arange(N) % period].contiguous())
    c = _raw_points_fwd(lib, packed, grid, period, rows, None, latent, N, train)
    d = _raw_points_fwd(lib, packed, tiled, 0, rows, None, latent, N, train)
    assert torch.equal(c[0], d[0]), "points_period differs from the points tiled on the host"
    assert not train or torch.equal(c[1], d[1]), "points_period: the activation images differ"
    assert not torch.equal(c[0], b[0])


# ---- F: latent sizes at the padding edges of the input block ---------------------------------------------------------------------
EDGE_LATENTS = (1, 5, 29, 30, 61)       # 3 + L against the multiples of 8 and of 32 the kernels pad it to


def body_latent_size(mode, latent):
    body = "F latent sizes"
    if mode == "points":
        case = _make_case(mode, 70 + latent, latent, N=130)
    else:
        case = _make_case(mode, 170 + latent, latent, runs=[40, 1, 64, 25])
    _with_references(case, 9)
    what = "%s L %d" % (mode, latent)
    net = _net_of(case)
    pts, z = OPS.dev(case.pts).requires_grad_(True), OPS.dev(case.z).requires_grad_(True)
    out = _run(net, case, pts, z)
    check_forward(body, out, case.r64["out"], what)
    grads = list(torch.autograd.grad(out, [pts, z] + list(net.parameters()), OPS.dev(case.dy)))
    check(body, grads.pop(0), case.r32["points"], case.r64["points"], what + " d points")
    check(body, grads.pop(0), case.r32["latents"], case.r64["latents"], what + " d latents")
    check_params(body, net, grads, case.r32, case.r64, what)


# ---- G: one shared grid for several shapes ---------------------------------------------------------------------------------------
SPHERE_POINTS = {8: 280, 16: 2320}      # grid points inside |p| < 1.1: no multiple of 128


def body_sphere_grids(R):
    from shapegan_amd.model import sdf_net as SN
    SN.sdf_voxelization_helper.clear()          # (its cached grids live on the device of whoever asked first)
    try:
        net = make_net(81, 32)
        z = OPS.dev(torch.randn(3, 32, generator=torch.Generator().manual_seed(82)) * 0.5)
        for kw in (dict(sphere_only=True), dict(sphere_only=False, pad=True)):
            grids = net.voxel_grids(z, R, **kw)
            edge = R if kw["sphere_only"] else R + 2
            assert tuple(grids.shape) == (3, edge, edge, edge)
            if kw["sphere_only"]:
                assert net._helper(R, True).point_count == SPHERE_POINTS[R]
            for s in range(3):
                one = torch.from_numpy(net.get_voxels(z[s], R, **kw))
                assert torch.equal(grids[s].cpu(), one), "voxel_grids differs from get_voxels for shape %d (%s)" % (s, kw)
    finally:
        SN.sdf_voxelization_helper.clear()


def body_grid_values():
    from shapegan_amd.util import get_voxel_coordinates
    body = "G shared grids"
    net = make_net(83, 32)
    sd = state_of(net)
    grid = torch.tensor(get_voxel_coordinates(8), dtype=torch.float32)
    cpu_pts = grid[grid.norm(dim=1) < 1.1].contiguous()
    assert cpu_pts.shape[0] == 280
    cpu_z = torch.randn(3, 32, generator=torch.Generator().manual_seed(84)) * 0.5
    pts, z = OPS.dev(cpu_pts), OPS.dev(cpu_z)
    got = net.grid_values(z, pts)
    assert tuple(got.shape) == (3, 280)
    with torch.no_grad():
        for s in range(3):
            assert torch.equal(got[s], net.forward_shapes(pts, z[s:s + 1], 280)), "grid_values differs from forward_shapes for shape %d" % s
    ref = O.sdfnet_forward({k: v.double() for k, v in sd.items()}, cpu_pts.double().repeat(3, 1), cpu_z.double().repeat_interleave(280, 0))
    check_forward(body, got, ref, "grid_values 3 x 280")


def body_points_per_shape_refusal():
    """The C ABI itself: two shapes of 280 points and no shape index is refused by the argument check (a 64-point tile would hold
    points of both shapes), by either library; with the shape index the same call runs."""
    import ctypes
    import shapegan_amd.lib as L
    from shapegan_amd.lib import check, f32c, ptr, stream
    lib = L.load()
    latent, S, pps = 32, 2, 280
    net = make_net(85, latent)
    params = [f32c(p.detach()) for p in net._params()]
    dev = params[0].device
    g = torch.Generator().manual_seed(86)
    pts, z = OPS.dev(torch.rand(pps, 3, generator=g) * 2 - 1), OPS.dev(torch.randn(S, latent, generator=g) * 0.5)
    packed = torch.empty(lib.sg_sdfnet_packed_floats(3), dtype=torch.float32, device=dev)
    zb1, zb5 = torch.empty((S, 256), dtype=torch.float32, device=dev), torch.empty((S, 256), dtype=torch.float32, device=dev)
    arr = (ctypes.c_void_p * 16)(*[ptr(p) for p in params])
    check(lib.sg_sdfnet_pack_shape_bias(arr, latent, ptr(packed), ptr(z), S, ptr(zb1), ptr(zb5), stream()), "sdfnet_pack_shape_bias")
    out = torch.zeros(S * pps, dtype=torch.float32, device=dev)

    def call(sid):
        return lib.sg_sdfnet_fwd(ptr(pts), pps, None, None, latent, ptr(packed), 3, ptr(zb1), ptr(zb5), pps, ptr(sid), ptr(out), None,
                                 S * pps, S * pps, stream())
    rc = call(None)
    assert rc != 0, "two shapes of 280 points without a shape index were accepted"
    with pytest.raises(RuntimeError, match="points_per_shape"):
        check(rc, "sdfnet_fwd")
    sid = torch.arange(S, dtype=torch.int32, device=dev).repeat_interleave(pps)
    check(call(sid), "sdfnet_fwd")
    with torch.no_grad():
        for s in range(S):
            assert torch.equal(out[s * pps:(s + 1) * pps], net.forward_shapes(pts, z[s:s + 1], pps))
