"""Inputs, float64 references, checks and test bodies for the point-GAN kernels in every calling form: the LayerNorm form of the
fused MLP (sg_sdfgen_pack / _fwd / _bwd / _bwd_finish, ops.SDFGenFused, SDFGenerator) and the fused PointNet selection pass
(sg_pointnet_select, ops.pointnet_select, the branches of PointNet.forward).  tests/test_gpu_pointgan_forms.py calls the bodies on
the GPU, tests/test_cpu_twin.py on the twin.  Pure Python: nothing here is a test by itself.

Reference.  oracle.torch_oracle (sdf_generator_forward, pointnet_forward, pointnet_features) on a float64 copy of the state and
the inputs, and again in float32; autograd of sum(out * dy) in each precision.

Criterion.  Gradients: test_gpu_modules.check_against_oracles at its defaults,
    |got - ref64| <= 1e-4 * mean|ref64| + 4 * max|ref32 - ref64|,   at most 0.1 % of the elements (or 4) beyond it, those within
    5 % of the tensor's largest entry.
Forward outputs: rtol 1e-4, atol 2e-6 against float64.

ReLU kinks (generator).  A point whose smallest float64 |ReLU input| over the seven normed layers is below 1e-6 gets no upstream
gradient (the share of such points is asserted to stay under 0.05); a point that carries a one-hot upstream gradient is redrawn
from its seed until the reference calls it safe.  Near-ties (PointNet).  The (sub)gradient through a max is undefined at a tie:
a body that checks a gradient through the max redraws each of its clouds from seed, seed + 1, ... (at most 20 draws) until, for
every channel of the cloud's float64 features, largest - second largest > 64 * max|features32 - features64| (the maximum over the
points of that cloud and channel: with the maximum over all channels no cloud of 1024 points passes, with that of the two values
compared alone one more often than here).  A body that checks values
only does not redraw: the selected point must hold features64[idx] >= max64 - (1e-5 |max64| + 1e-6).  All of these decisions use
the references alone.

Every check prints `[pointgan-forms] body | what | err/tol | elements beyond tol` before it asserts; WORST keeps the largest
err / tol per body, STATS the largest kink share and the number of redraws per body."""
import ctypes
import functools

import pytest
import torch

import test_gpu_modules as M
import test_gpu_ops as OPS
from oracle import torch_oracle as O

WORST = {}
STATS = {}
FRAGILE_BELOW = 1e-6
FRAGILE_CAP = 0.05
TIE_FACTOR = 64.0
TIE_DRAWS = 20
SG_ERR_ARG = -1


# ---- checks --------------------------------------------------------------------------------------------------------------------
def _note(body, what, ratio, beyond, numel):
    print("[pointgan-forms] %s | %s | err/tol %.3g | %d of %d beyond tol" % (body, what, ratio, beyond, numel))
    WORST[body] = max(WORST.get(body, 0.0), ratio)


def _stat(body, share=None, redraws=None):
    s = STATS.setdefault(body, dict(kink_share=0.0, redraws=0))
    if share is not None:
        s["kink_share"] = max(s["kink_share"], share)
    if redraws is not None:
        s["redraws"] += redraws
    print("[pointgan-forms] %s | kink share %.4f | redraws %d" % (body, s["kink_share"], s["redraws"]))


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
    bound = 2e-6 + OPS.RTOL * ref.abs()
    _note(body, what + " (forward)", float(((got - ref).abs() / bound).max()), int(((got - ref).abs() > bound).sum()), got.numel())
    OPS.close(got, ref, atol=2e-6, what=what + " forward")


class _Calls(object):
    """Stands in for the library object the shells call: notes every entry point they call, with its arguments."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def noted(*args):
            self.calls.append((name, args))
            return fn(*args)
        return noted

    def names(self):
        return [c[0] for c in self.calls]

    def args_of(self, name):
        found = [c[1] for c in self.calls if c[0] == name]
        assert len(found) == 1, "%s was called %d times" % (name, len(found))
        return found[0]


class _recorded(object):
    """with _recorded() as rec: every library call the shells make inside is in rec.calls."""

    def __enter__(self):
        from shapegan_amd import ops
        self.ops, self.real = ops, ops._lib
        rec = _Calls(ops._lib())
        ops._lib = lambda: rec
        return rec

    def __exit__(self, *exc):
        self.ops._lib = self.real


def function_node(out):
    """The autograd node of ops.SDFGenFused behind `out` (the module reshapes what the Function returns)."""
    node = out.grad_fn
    while node is not None and not hasattr(node, "_forward_cls"):
        node = node.next_functions[0][0]
    assert node is not None, "no custom Function behind the output"
    return node


# ---- the LayerNorm form of the fused MLP: nets, references ------------------------------------------------------------------------
GEN_KEYS_UNUSED = ("norms.7.weight", "norms.7.bias")      # LayerNorm(1) behind the last layer: never used


def make_generator(seed, eps=None):
    """SDFGenerator(128, 256, 8) with non-trivial LayerNorm weights / biases, on the device the bodies run on (OPS.DEV is "cpu"
    under test_cpu_twin's on_cpu fixture)."""
    from shapegan_amd.model.point_sdf_net import SDFGenerator
    torch.manual_seed(seed)
    G = SDFGenerator(128, 256, 8, True, dropout=0.0)
    with torch.no_grad():
        for n in G.norms:
            n.weight.uniform_(0.5, 1.5)
            n.bias.uniform_(-0.3, 0.3)
    if eps is not None:
        for n in G.norms:
            n.eps = eps
    return G.to(OPS.DEV)


def state_of(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def gen_fragile(sd, pos, z, eps):
    P = {k: v.double() for k, v in sd.items()}
    return O.sdf_generator_min_preactivation(P, pos.double(), z.double(), eps) < FRAGILE_BELOW


def gen_reference(sd, pos, z, dy, dtype, eps):
    """out [S, pps] and the gradients of sum(out * dy) in `dtype`: dict(out, pos, z, params{name})."""
    P = O.clone_state({k: v.to(dtype) for k, v in sd.items()})
    p = pos.to(dtype).clone().requires_grad_(True)
    zz = z.to(dtype).clone().requires_grad_(True)
    out = O.sdf_generator_forward(P, p, zz, eps=eps).squeeze(-1)
    (out * dy.to(dtype)).sum().backward()
    return dict(out=out.detach(), pos=p.grad, z=zz.grad, params={k: v.grad for k, v in P.items()})


def gen_references(sd, pos, z, dy, eps):
    return gen_reference(sd, pos, z, dy, torch.float32, eps), gen_reference(sd, pos, z, dy, torch.float64, eps)


def masked_upstream(body, sd, pos, z, eps, seed):
    """A random upstream gradient [S, pps], zero on the points the float64 reference calls fragile."""
    fragile = gen_fragile(sd, pos, z, eps)
    share = float(fragile.float().mean())
    _stat(body, share=share)
    assert share < FRAGILE_CAP, "%.4f of the points sit on a ReLU kink" % share
    dy = torch.randn(pos.shape[:2], generator=torch.Generator().manual_seed(seed))
    dy[fragile] = 0
    return dy


class Case(object):
    """Inputs and references of one case: made once, shared by the bodies that need them, never written."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _tweak_offset_rows(G):
    with torch.no_grad():
        G.z_lin1.bias.add_(30.0)
        G.lins[4].bias.add_(30.0)


@functools.lru_cache(maxsize=None)
def _gen_case(body, seed, S, pps, eps=1e-5, offset_rows=False, with_references=True):
    G = make_generator(seed, eps)
    if offset_rows:
        _tweak_offset_rows(G)
    sd = state_of(G)
    g = torch.Generator().manual_seed(seed + 1)
    pos = torch.rand(S, pps, 3, generator=g) * 2 - 1
    z = torch.randn(S, 128, generator=g)
    case = Case(seed=seed, S=S, pps=pps, N=S * pps, eps=eps, sd=sd, pos=pos, z=z)
    if with_references:
        case.dy = masked_upstream(body, sd, pos, z, eps, seed + 2)
        case.r32, case.r64 = gen_references(sd, pos, z, case.dy, eps)
    return case


def _generator_of(case):
    G = make_generator(case.seed, case.eps)
    G.load_state_dict(case.sd)
    return G


def gen_param_names(G):
    return [k for k, _ in G.named_parameters() if k not in GEN_KEYS_UNUSED]


def check_gen_params(body, names, grads, r32, r64, what):
    for k, g in zip(names, grads):
        check(body, g, r32["params"][k], r64["params"][k], "%s grad %s" % (what, k))


def expects_shape_index(S, pps):
    """ops.SDFGenFused names every point's shape unless no tile can straddle two shapes."""
    return not (pps % 128 == 0 or pps >= S * pps)


def _fused_forward(G, pos, z):
    """G(pos, z) with the library calls noted: the fused entry must have been the one that ran."""
    with _recorded() as rec:
        out = G(pos, z)
    assert "sg_sdfgen_fwd" in rec.names(), "the call did not take the one-launch form"
    return out, rec


# ---- 1: shapes ------------------------------------------------------------------------------------------------------------------
# (S, pps, shape_index expected)
SMALL_SHAPES = [(1, 1, False), (1, 31, False), (1, 33, False), (40, 1, True), (7, 50, True), (300, 7, True), (3, 129, True),
                (2, 1056, True)]
SMALL_TILE_SHAPES = [(1, 16450, False), (129, 128, False), (329, 50, True)]
SHAPES = SMALL_SHAPES + SMALL_TILE_SHAPES


def body_shapes(S, pps, sid_expected):
    """Output, every parameter gradient except norms.7 and the z gradient at one shape.

    The forward's plan is tile_plan(N, 64, 512): tiles = ceil(N / 64), full = tiles // 512 * 512, rem = tiles - full; when
    256 < rem <= 384 it launches full + 256 tiles of 64 points and ceil((N - 64 (full + 256)) / 32) tiles of 32.
      (1, 16450) and (329, 50): N = 16450, tiles = 258, full = 0, rem = 258 -> 256 big tiles (points 0 .. 16383) + ceil(66 / 32) = 3
        small ones, the last holding 2 points;
      (129, 128): N = 16512, tiles = 258 -> 256 big + 128 / 32 = 4 small ones.
    Every smaller case has tiles <= 33: one partial round (full == 0, rem <= 256), big tiles only.  The backward runs 32-point
    tiles throughout (ceil(N / 32) of them; more than 64 make more than one finish split: (2, 1056) has 66)."""
    import shapegan_amd.lib as L
    body = "1 shapes"
    N = S * pps
    what = "%d x %d" % (S, pps)
    assert expects_shape_index(S, pps) == sid_expected
    blocks = L.load().sg_sdfnet_bwd_blocks(N)
    if N > 16384:
        nsmall = {16450: 3, 16512: 4}[N]
        assert blocks == 256 + nsmall, "%s: the forward's plan has %d tiles, not 256 of 64 points + %d of 32" % (what, blocks, nsmall)
        assert L.load().sg_sdfnet_bwd_tile_start(N, 256) == 16384 and L.load().sg_sdfnet_bwd_tile_start(N, 257) == 16384 + 32
    else:
        assert blocks == (N + 63) // 64, what + ": small tiles in a case meant to run big tiles only"
    if (S, pps) == (2, 1056):
        assert L.load().sg_sdfgen_bwd_blocks(N) == 66
    case = _gen_case(body, 100 + S + pps, S, pps)
    G = _generator_of(case)
    pos, z = OPS.dev(case.pos), OPS.dev(case.z).requires_grad_(True)
    out, rec = _fused_forward(G, pos, z)
    args = rec.args_of("sg_sdfgen_fwd")
    assert (args[5] is not None) == sid_expected, what + ": shape_index " + ("missing" if sid_expected else "passed")
    assert args[4] == pps and args[9] == N and args[10] == N and args[8] is not None
    check_forward(body, out, case.r64["out"], what)
    names = gen_param_names(G)
    params = dict(G.named_parameters())
    grads = list(torch.autograd.grad(out, [z] + [params[k] for k in names], OPS.dev(case.dy).reshape(out.shape)))
    gz = grads.pop(0)
    if S <= 40:
        for s in range(S):       # row by row: a wrong short segment must not hide behind the others
            check(body, gz[s], case.r32["z"][s], case.r64["z"][s], what + " d z row %d" % s)
    check(body, gz, case.r32["z"], case.r64["z"], what + " d z")
    check_gen_params(body, names, grads, case.r32, case.r64, what)


# ---- 2: one-hot upstream gradients -------------------------------------------------------------------------------------------------
ONE_HOT_S, ONE_HOT_PPS = 329, 50
ONE_HOT_POSITIONS = {"first": 0, "p31": 31, "p32": 32, "shape_last": 100 * 50 + 49, "shape_first": 101 * 50, "last_big": 16383,
                     "first_small": 16384, "last": ONE_HOT_S * ONE_HOT_PPS - 1}


def body_one_hot(where):
    """Upstream gradient 1 on one point of 329 x 50: the gradients against the reference of that point alone; the z gradient rows
    of every other shape are exactly zero."""
    body = "2 one-hot"
    case = _gen_case(body, 201, ONE_HOT_S, ONE_HOT_PPS, with_references=False)
    i = ONE_HOT_POSITIONS[where]
    s, q = divmod(i, ONE_HOT_PPS)
    g = torch.Generator().manual_seed(7000 + i)
    redraws = -1
    while True:
        xyz = torch.rand(1, 1, 3, generator=g) * 2 - 1
        redraws += 1
        if not bool(gen_fragile(case.sd, xyz, case.z[s:s + 1], case.eps)[0, 0]):
            break
    _stat(body, redraws=redraws)
    r32, r64 = gen_references(case.sd, xyz, case.z[s:s + 1], torch.ones(1, 1), case.eps)
    cpu_pos = case.pos.clone()
    cpu_pos[s, q] = xyz[0, 0]
    dy = torch.zeros(case.N)
    dy[i] = 1.0
    G = _generator_of(case)
    pos, z = OPS.dev(cpu_pos), OPS.dev(case.z).requires_grad_(True)
    out, _ = _fused_forward(G, pos, z)
    what = "one-hot %s (point %d, shape %d)" % (where, i, s)
    check_forward(body, out.reshape(-1)[i:i + 1], r64["out"], what)
    names = gen_param_names(G)
    params = dict(G.named_parameters())
    grads = list(torch.autograd.grad(out, [z] + [params[k] for k in names], OPS.dev(dy).reshape(out.shape)))
    gz = grads.pop(0).detach().cpu()
    check(body, gz[s], r32["z"][0], r64["z"][0], what + " d z row")
    others = torch.ones(case.S, dtype=torch.bool)
    others[s] = False
    assert not bool(gz[others].ne(0).any()), what + ": the z row of a shape without upstream gradient is not exactly zero"
    check_gen_params(body, names, grads, r32, r64, what)


# ---- 3: which inputs require grad --------------------------------------------------------------------------------------------------
SUBSETS = [(z, l, n) for z in (True, False) for l in (True, False) for n in (True, False) if z or l or n]


def _case_small():
    return _gen_case("1 shapes", 100 + 7 + 50, 7, 50)


def _is_norm(name):
    return name.startswith("norms.")


def body_which_grads(need_z, need_lins, need_norms):
    """z / the Linear layers (lins.*, z_lin1, z_lin2) / the LayerNorm parameters require grad in every combination: what was not
    asked for is None from SDFGenFused.backward itself, the rest matches float64."""
    body = "3 which-grads"
    case = _case_small()
    what = "z%d lins%d norms%d" % (need_z, need_lins, need_norms)
    G = _generator_of(case)
    for k, p in G.named_parameters():
        p.requires_grad_(need_norms if _is_norm(k) else need_lins)
    pos, z = OPS.dev(case.pos), OPS.dev(case.z).requires_grad_(need_z)
    out, _ = _fused_forward(G, pos, z)
    check_forward(body, out, case.r64["out"], what)
    dy = OPS.dev(case.dy)
    # the Function's inputs: cache, pos, zb1, zb5, pps, eps, grad_mode, lins.{0..7}.{weight,bias}, norms.{0..6}.{weight,bias}
    raw = function_node(out).apply(dy.reshape(-1))
    assert len(raw) == 37
    assert all(raw[i] is None for i in (0, 1, 4, 5, 6)), what + ": a gradient for an input that is no tensor, or for pos"
    rows_live = need_z or need_lins           # zb1 / zb5 come from z and from z_lin*, lins.0.bias / lins.4.bias
    assert (raw[2] is not None) == rows_live and (raw[3] is not None) == rows_live, what + ": the gradients of the per-shape rows"
    for i in range(16):
        expected = need_lins and i not in (1, 9)      # lins.0.bias / lins.4.bias receive theirs through the rows
        assert (raw[7 + i] is not None) == expected, what + ": gradient of Linear tensor %d %s" % (i, "missing" if expected else "returned")
    for i in range(14):
        assert (raw[23 + i] is not None) == need_norms, what + ": gradient of LayerNorm tensor %d" % i
    names = [k for k in gen_param_names(G) if (need_norms if _is_norm(k) else need_lins)]
    params = dict(G.named_parameters())
    grads = list(torch.autograd.grad(out, ([z] if need_z else []) + [params[k] for k in names], dy.reshape(out.shape)))
    if need_z:
        check(body, grads.pop(0), case.r32["z"], case.r64["z"], what + " d z")
    check_gen_params(body, names, grads, case.r32, case.r64, what)


def body_no_grad_forward():
    """The forward without activation images (acts == NULL): under torch.no_grad(), and as the Function called with grad_mode
    False, through which a backward raises."""
    from shapegan_amd import ops
    body = "3 which-grads"
    case = _case_small()
    G = _generator_of(case)
    pos, z = OPS.dev(case.pos), OPS.dev(case.z)
    with torch.no_grad():
        out, rec = _fused_forward(G, pos, z)
    assert rec.args_of("sg_sdfgen_fwd")[8] is None, "a forward under no_grad kept activation images"
    assert out.grad_fn is None
    check_forward(body, out, case.r64["out"], "forward under no_grad")
    with torch.no_grad():
        zb1 = ops.linear(z, G.z_lin1.weight, G.z_lin1.bias + G.lins[0].bias)
        zb5 = ops.linear(z, G.z_lin2.weight, G.z_lin2.bias + G.lins[4].bias)
    params = [t for lin in G.lins for t in (lin.weight, lin.bias)] + [t for n in G.norms[:7] for t in (n.weight, n.bias)]
    with _recorded() as rec:
        raw = ops.SDFGenFused.apply(G._pack, pos.reshape(-1, 3), zb1, zb5, case.pps, case.eps, False, *params)
    assert rec.args_of("sg_sdfgen_fwd")[8] is None
    assert torch.equal(raw, out.reshape(-1)), "grad_mode False computes another output than no_grad"
    assert raw.requires_grad
    with pytest.raises(RuntimeError, match="without grad mode"):
        raw.sum().backward()


# ---- 4: positions that require grad -------------------------------------------------------------------------------------------------
def body_positions_require_grad():
    """pos.requires_grad_(): the module returns d out / d pos (the fused backward has none: the call runs layer by layer), and the
    parameter and z gradients of that call."""
    body = "4 positions"
    case = _gen_case(body, 401, 3, 129)
    G = _generator_of(case)
    pos, z = OPS.dev(case.pos).requires_grad_(True), OPS.dev(case.z).requires_grad_(True)
    out = G(pos, z)
    check_forward(body, out, case.r64["out"], "3 x 129")
    names = gen_param_names(G)
    params = dict(G.named_parameters())
    grads = list(torch.autograd.grad(out, [pos, z] + [params[k] for k in names], OPS.dev(case.dy).reshape(out.shape), allow_unused=True))
    assert grads[0] is not None, "the gradient with respect to pos was dropped"
    assert float(case.r64["pos"].abs().max()) > 0.01
    check(body, grads.pop(0), case.r32["pos"], case.r64["pos"], "d pos")
    check(body, grads.pop(0), case.r32["z"], case.r64["z"], "d z")
    check_gen_params(body, names, grads, case.r32, case.r64, "pos requires grad")
    with torch.no_grad():       # nothing to return a position gradient to: the one-launch form
        _fused_forward(G, pos, z)


# ---- 5 / 6: rows whose mean dwarfs their spread; a non-default eps --------------------------------------------------------------------
def _body_all_grads(body, case, what):
    G = _generator_of(case)
    pos, z = OPS.dev(case.pos), OPS.dev(case.z).requires_grad_(True)
    out, rec = _fused_forward(G, pos, z)
    assert abs(rec.args_of("sg_sdfgen_fwd")[6] - case.eps) <= 1e-7 * case.eps
    check_forward(body, out, case.r64["out"], what)
    names = gen_param_names(G)
    params = dict(G.named_parameters())
    grads = list(torch.autograd.grad(out, [z] + [params[k] for k in names], OPS.dev(case.dy).reshape(out.shape)))
    check(body, grads.pop(0), case.r32["z"], case.r64["z"], what + " d z")
    check_gen_params(body, names, grads, case.r32, case.r64, what)


def body_offset_rows():
    """z_lin1.bias += 30, lins.4.bias += 30: the inputs of LayerNorm 0 and 4 have a row mean far above the row's spread, where
    E[x^2] - E[x]^2 would cancel and where an accumulator started from the bias row rounds every product it adds to the ulp of 30.
    Same criterion as everywhere: only the float32 oracle's own loss (the 4 |ref32 - ref64| term) widens it."""
    body = "5 offset rows"
    case = _gen_case(body, 501, 3, 129, offset_rows=True)
    assert float(case.sd["z_lin1.bias"].mean()) > 29 and float(case.sd["lins.4.bias"].mean()) > 29
    _body_all_grads(body, case, "rows offset by 30")


def body_eps(eps):
    body = "6 eps"
    case = _gen_case(body, 601, 7, 50, eps=eps)
    ref_default = O.sdf_generator_forward({k: v.double() for k, v in case.sd.items()}, case.pos.double(), case.z.double()).squeeze(-1)
    assert float((ref_default - case.r64["out"]).abs().max()) > 1e-4, "eps does not move the reference: the case checks nothing"
    _body_all_grads(body, case, "eps %g" % eps)


# ---- 7: the C ABI with ldn > N -------------------------------------------------------------------------------------------------------
def _gen_reference_with_rows(sd, pos, z, dy, dtype):
    """gen_reference plus the gradients of the per-shape rows zb1 / zb5 ([S, 256] each): two extra latent blocks e1 = e5 = 0 that
    z_lin1 / z_lin2 pass through unchanged (identity columns), so d / d e1 = d / d zb1 and the forward adds exact zeros."""
    S = z.shape[0]
    P = {k: v.to(dtype) for k, v in sd.items()}
    eye, zero = torch.eye(256, dtype=dtype), torch.zeros(256, 256, dtype=dtype)
    P["z_lin1.weight"] = torch.cat([P["z_lin1.weight"], eye, zero], dim=1)
    P["z_lin2.weight"] = torch.cat([P["z_lin2.weight"], zero, eye], dim=1)
    P = O.clone_state(P)
    e = torch.zeros(S, 512, dtype=dtype, requires_grad=True)
    out = O.sdf_generator_forward(P, pos.to(dtype), torch.cat([z.to(dtype), e], dim=1)).squeeze(-1)
    (out * dy.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in P.items()}
    return dict(out=out.detach(), params=grads, t1=e.grad[:, :256].t().contiguous(), t5=e.grad[:, 256:].t().contiguous())


def body_raw_abi_ldn():
    """sg_sdfgen_fwd / _bwd / _bwd_finish with a leading dimension ldn = N + 37 of the activation and dZ images (no shell passes
    one), N = 2100 = 300 x 7: out, the seven bias gradients, w8 / b8, the point columns of dW1 / dW5, the 14 LayerNorm gradients and
    the per-shape sums t1 / t5 against float64; and the refusals the source states, each SG_ERR_ARG with nothing written."""
    import shapegan_amd.lib as L
    from shapegan_amd.lib import check as rc_check, f32c, ptr, stream, tickets, workspace
    body = "7 raw ABI"
    lib = L.load()
    S, pps, eps = 300, 7, 1e-5
    N = S * pps
    ldn = N + 37
    case = _gen_case(body, 701, S, pps, with_references=False)
    dy = masked_upstream(body, case.sd, case.pos, case.z, eps, 703)
    r32, r64 = (_gen_reference_with_rows(case.sd, case.pos, case.z, dy, dt) for dt in (torch.float32, torch.float64))
    G = _generator_of(case)
    held = [f32c(t.detach()) for lin in G.lins for t in (lin.weight, lin.bias)] + \
           [f32c(t.detach()) for n in G.norms[:7] for t in (n.weight, n.bias)]
    dev = held[0].device
    packed = torch.empty(lib.sg_sdfnet_packed_floats(3), dtype=torch.float32, device=dev)
    rc_check(lib.sg_sdfgen_pack((ctypes.c_void_p * 16)(*[ptr(t) for t in held[:16]]), (ctypes.c_void_p * 14)(*[ptr(t) for t in held[16:]]),
                                ptr(packed), stream()), "sdfgen_pack")
    sd = case.sd
    zb1 = OPS.dev(torch.nn.functional.linear(case.z, sd["z_lin1.weight"], sd["z_lin1.bias"] + sd["lins.0.bias"]).contiguous())
    zb5 = OPS.dev(torch.nn.functional.linear(case.z, sd["z_lin2.weight"], sd["z_lin2.bias"] + sd["lins.4.bias"]).contiguous())
    pos = OPS.dev(case.pos.reshape(N, 3).contiguous())
    sid = OPS.dev(torch.arange(S, dtype=torch.int32).repeat_interleave(pps).contiguous())
    gout = OPS.dev(dy.reshape(N).contiguous())
    marker = -7.0
    out = torch.full((N,), marker, dtype=torch.float32, device=dev)
    acts = torch.zeros(lib.sg_sdfgen_acts_floats(ldn), dtype=torch.float32, device=dev)

    def fwd(pps_, sid_, eps_, acts_, ldn_):
        return lib.sg_sdfgen_fwd(ptr(pos), ptr(packed), ptr(zb1), ptr(zb5), pps_, ptr(sid_), eps_, ptr(out), ptr(acts_), ldn_, N, stream())
    # the refusals, before any launch: out keeps its marker
    assert fwd(pps, sid, eps, acts, N - 1) == SG_ERR_ARG, "ldn < N was accepted"
    assert fwd(pps, None, eps, acts, ldn) == SG_ERR_ARG, "7 points per shape without a shape index were accepted"
    assert fwd(pps, sid, 0.0, acts, ldn) == SG_ERR_ARG and fwd(pps, sid, -1e-5, acts, ldn) == SG_ERR_ARG, "eps <= 0 was accepted"
    assert bool((out == marker).all()) and not bool(acts.ne(0).any()), "a refused call wrote"
    rc_check(fwd(pps, sid, eps, acts, ldn), "sdfgen_fwd")
    check_forward(body, out, r64["out"], "ldn = N + 37")
    dz = torch.zeros(7 * 256 * ldn + 32, dtype=torch.float32, device=dev)[:7 * 256 * ldn].view(7, 256, ldn)
    dz8 = torch.zeros(N, dtype=torch.float32, device=dev)
    nblk = lib.sg_sdfgen_bwd_blocks(N)
    assert nblk == 66      # two finish splits
    part_row = L.abi.DEFINES["SG_SDFGEN_PARTIAL_ROW"]
    bsum = torch.zeros((nblk, part_row), dtype=torch.float32, device=dev)

    def bwd(ldn_):
        return lib.sg_sdfgen_bwd(ptr(gout), ptr(acts), ptr(dz), ptr(dz8), ptr(bsum), ptr(pos), ptr(packed), ldn_, N, stream())
    assert bwd(N - 1) == SG_ERR_ARG and not bool(dz8.ne(0).any()), "sg_sdfgen_bwd: ldn < N was accepted"
    rc_check(bwd(ldn), "sdfgen_bwd")
    assert torch.equal(dz8, gout)
    bias = [torch.zeros(256, dtype=torch.float32, device=dev) for _ in range(7)]
    norm = [torch.zeros(256, dtype=torch.float32, device=dev) for _ in range(14)]
    w8, b8 = torch.zeros(256, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
    w1, w5 = torch.zeros((256, 3), dtype=torch.float32, device=dev), torch.zeros((256, 259), dtype=torch.float32, device=dev)
    t1, t5 = torch.zeros((256, S), dtype=torch.float32, device=dev), torch.zeros((256, S), dtype=torch.float32, device=dev)
    seg_off = OPS.dev(torch.arange(S + 1, dtype=torch.int64) * pps)
    ws = workspace("sdfgen_finish", lib.sg_sdfgen_bwd_finish_workspace_bytes(N), dev)
    tk = tickets("sdfgen_finish", dev, 32)
    barr, narr = (ctypes.c_void_p * 7)(*[ptr(t) for t in bias]), (ctypes.c_void_p * 14)(*[ptr(t) for t in norm])

    def finish(ldn_):
        return lib.sg_sdfgen_bwd_finish(ptr(dz), ptr(bsum), ldn_, N, barr, ptr(w8), ptr(b8), ptr(w1), 3, ptr(w5) + 4 * 256, 259, narr,
                                        ptr(seg_off), S, ptr(t1), ptr(t5), ptr(ws), ws.numel(), ptr(tk), stream())
    assert finish(N - 1) == SG_ERR_ARG and not bool(t1.ne(0).any()), "sg_sdfgen_bwd_finish: ldn < N was accepted"
    rc_check(finish(ldn), "sdfgen_bwd_finish")
    assert not bool(tk.ne(0).any()), "the finishing launch left its tickets non-zero"

    def ref(name):
        return r32["params"][name], r64["params"][name]
    for g in range(7):        # row sums of dZ_{g+1}: lins.g.bias (layers 0 and 4: the sum of the per-shape row gradients)
        check(body, bias[g], *ref("lins.%d.bias" % g), what="bias gradient %d" % g)
    check(body, w8.reshape(1, 256), *ref("lins.7.weight"), what="w8 gradient")
    check(body, b8, *ref("lins.7.bias"), what="b8 gradient")
    check(body, w1, *ref("lins.0.weight"), what="dW1 point columns")
    a32, a64 = ref("lins.4.weight")
    check(body, w5[:, 256:], a32[:, 256:], a64[:, 256:], what="dW5 point columns")
    assert not bool(w5[:, :256].ne(0).any()), "the finishing launch wrote dW5 outside its point columns"
    for l in range(7):
        check(body, norm[l], *ref("norms.%d.weight" % l), what="LayerNorm %d weight gradient" % l)
        check(body, norm[7 + l], *ref("norms.%d.bias" % l), what="LayerNorm %d bias gradient" % l)
    check(body, t1, r32["t1"], r64["t1"], what="t1")
    check(body, t5, r32["t5"], r64["t5"], what="t5")


# ---- PointNet: nets, references -----------------------------------------------------------------------------------------------------
def make_critic(seed):
    from shapegan_amd.model.point_sdf_net import PointNet
    torch.manual_seed(seed)
    return PointNet(out_channels=1).to(OPS.DEV)


def draw_clouds(seed, lead, P):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.rand(tuple(lead) + (P, 3), generator=g) * 2 - 1, torch.rand(tuple(lead) + (P, 1), generator=g) * 0.2 - 0.1], -1)


def features(sd, x, dtype):
    with torch.no_grad():
        return O.pointnet_features({k: v.to(dtype) for k, v in sd.items()}, x.to(dtype))


def has_near_tie(sd, cloud):
    """Whether some channel of one cloud [P, 4] has the two largest of its float64 features within 64 x the float32 oracle's own
    error on that channel's points of each other."""
    f64, f32 = features(sd, cloud, torch.float64), features(sd, cloud, torch.float32)
    top = f64.topk(2, dim=0).values
    return bool((top[0] - top[1] <= TIE_FACTOR * (f32.double() - f64).abs().amax(dim=0)).any())


def clouds_without_near_tie(body, sd, seed, lead, P):
    """Clouds [lead..., P, 4], every one redrawn from its own seeds (seed + 100 c, + 1, ...) until it has no near-tie: the rule
    speaks of every (cloud, channel), so the draws of one cloud do not depend on the others."""
    count = 1
    for n in lead:
        count *= n
    clouds, redraws = [], 0
    for c in range(count):
        for draw in range(TIE_DRAWS):
            x = draw_clouds(seed + 100 * c + draw, (), P)
            if not has_near_tie(sd, x):
                break
        else:
            raise AssertionError("%s: cloud %d of %d points has a near-tie of its two largest features in each of %d draws" % (
                body, c, P, TIE_DRAWS))
        clouds.append(x)
        redraws += draw
    _stat(body, redraws=redraws)
    return torch.stack(clouds).reshape(tuple(lead) + (P, 4))


def critic_reference(sd, x, dy, dtype):
    """out and the gradients of sum(out * dy): dict(out, pos, dist, params{name})."""
    P = O.clone_state({k: v.to(dtype) for k, v in sd.items()})
    pos, dist = x[..., :3].to(dtype).clone().requires_grad_(True), x[..., 3:].to(dtype).clone().requires_grad_(True)
    out = O.pointnet_forward(P, pos, dist)
    (out * dy.to(dtype)).sum().backward()
    return dict(out=out.detach(), pos=pos.grad, dist=dist.grad, params={k: v.grad for k, v in P.items()})


def _critic_of(sd, seed):
    D = make_critic(seed)
    D.load_state_dict(sd)
    return D


def _nn1_args(D):
    lins = [m for m in D.nn1 if isinstance(m, torch.nn.Linear)]
    return [l.weight for l in lins], [l.bias for l in lins]


# ---- 8: the selection pass ------------------------------------------------------------------------------------------------------------
# (B, P, twin rows): P / 32 = 1, 2, 13, 16, 17 and 257 tiles per cloud (the merge runs 4 phases x 4 tiles in flight)
SELECT_CASES = [(2, 32, False), (2, 64, False), (2, 64, True), (2, 416, False), (2, 512, False), (2, 544, False), (1, 8224, False)]


def body_select(B, P, twin_rows):
    """ops.pointnet_select against the float64 features: the maxima (rtol 1e-5, atol 1e-6), and the selected point by what it holds
    in float64.  twin_rows: points 5 and 21 of every cloud are identical; a channel that selects either reports 5."""
    from shapegan_amd import ops
    body = "8 select"
    what = "%d x %d%s" % (B, P, " twin rows" if twin_rows else "")
    D = make_critic(800 + P)
    sd = state_of(D)
    x = draw_clouds(801 + P, (B,), P)
    if twin_rows:
        x[:, 21] = x[:, 5]
    f64 = features(sd, x, torch.float64)
    max64, arg64 = f64.max(dim=1)
    weights, biases = _nn1_args(D)
    out, idx = ops.pointnet_select(D._pack, OPS.dev(x), weights, biases)
    assert tuple(out.shape) == (B, 512) and tuple(idx.shape) == (B, 512) and idx.dtype == torch.int32
    got, sel = out.detach().cpu(), idx.detach().cpu().long()
    bound = 1e-6 + 1e-5 * max64.abs()
    err = (got.double() - max64).abs()
    _note(body, what + " maxima", float((err / bound).max()), int((err > bound).sum()), got.numel())
    OPS.close(got, max64.float(), rtol=1e-5, atol=1e-6, what=what + " maxima")
    assert int(sel.min()) >= 0 and int(sel.max()) < P, what + ": a selected point outside the cloud"
    deficit = max64 - f64.gather(1, sel.unsqueeze(1)).squeeze(1)
    _note(body, what + " selected point", float((deficit / bound).max()), int((deficit > bound).sum()), sel.numel())
    assert bool((deficit <= bound).all()), what + ": a selected point holds less than the maximum by %.3g of the bound" % float(
        (deficit / bound).max())
    if twin_rows:
        assert int(((arg64 == 5) | (arg64 == 21)).sum()) > 0, "no channel has its maximum at the twin rows: the case checks nothing"
        assert bool((sel == 5).any()), what + ": no channel selected the twin rows although float64 has maxima there"
        assert not bool((sel == 21).any()), what + ": a tie was given to the higher point"
    assert torch.equal(D.selected_points(OPS.dev(x)).cpu(), sel)


# ---- 9: every branch of PointNet.forward on the same inputs -----------------------------------------------------------------------------
FORWARD_POINTS = (50, 64, 1024, 1030)


@functools.lru_cache(maxsize=None)
def _critic_case(body, P, lead):
    seed = 900 + P + 7 * len(lead)
    sd = state_of(make_critic(seed))
    x = clouds_without_near_tie(body, sd, seed + 1, lead, P)
    dy = torch.randn(tuple(lead) + (1,), generator=torch.Generator().manual_seed(seed + 2))
    r32, r64 = critic_reference(sd, x, dy, torch.float32), critic_reference(sd, x, dy, torch.float64)
    return Case(seed=seed, sd=sd, x=x, dy=dy, r32=r32, r64=r64, P=P, lead=lead)


def _check_critic_grads(body, D, out, pos, dist, case, what):
    params = list(D.named_parameters())
    grads = list(torch.autograd.grad(out, [pos, dist] + [p for _, p in params], OPS.dev(case.dy).reshape(out.shape)))
    check(body, grads.pop(0).reshape(case.r64["pos"].shape), case.r32["pos"], case.r64["pos"], what + " d pos")
    check(body, grads.pop(0).reshape(case.r64["dist"].shape), case.r32["dist"], case.r64["dist"], what + " d dist")
    for (k, _), g in zip(params, grads):
        check(body, g, case.r32["params"][k], case.r64["params"][k], "%s grad %s" % (what, k))


def body_forward_forms(P):
    """The same weights and clouds through every branch of PointNet.forward that P admits, each against pointnet_forward in
    float64; the recorded ones with every parameter gradient, d / d dist and d / d pos."""
    from shapegan_amd.model.point_sdf_net import PointNet
    body = "9 forward forms"
    assert PointNet.SPARSE_MIN_POINTS == 1024      # P = 64 / 1024 stand on the two sides of it
    case = _critic_case(body, P, (2,))
    D = _critic_of(case.sd, case.seed)
    cpu_pos, cpu_dist = case.x[..., :3].contiguous(), case.x[..., 3:].contiguous()
    # nothing to record: the fused selection pass for whole 32-point tiles, the dense layers otherwise
    with torch.no_grad(), _recorded() as rec:
        out = D(OPS.dev(cpu_pos), OPS.dev(cpu_dist))
    assert ("sg_pointnet_select" in rec.names()) == (P % 32 == 0), "P %d without grad: %s" % (P, rec.names())
    assert ("sg_segmax_fwd" in rec.names()) == (P % 32 != 0)
    check_forward(body, out, case.r64["out"], "P %d no-grad" % P)
    # recorded: dense below SPARSE_MIN_POINTS, from there on the selected points (found by the fused pass or by SegMax)
    pos, dist = OPS.dev(cpu_pos).requires_grad_(True), OPS.dev(cpu_dist).requires_grad_(True)
    with _recorded() as rec:
        out = D(pos, dist)
    sparse = P >= 1024
    assert ("sg_gather_rows" in rec.names()) == sparse and ("sg_rowdot" in rec.names()) == sparse, "P %d recorded: %s" % (P, rec.names())
    assert ("sg_pointnet_select" in rec.names()) == (sparse and P % 32 == 0)
    assert ("sg_segmax_fwd" in rec.names()) == (not sparse or P % 32 != 0)
    what = "P %d recorded %s" % (P, "sparse" if sparse else "dense")
    check_forward(body, out, case.r64["out"], what)
    _check_critic_grads(body, D, out, pos, dist, case, what)
    # the ragged form on the flattened clouds
    pos, dist = OPS.dev(cpu_pos.reshape(-1, 3)).requires_grad_(True), OPS.dev(cpu_dist.reshape(-1, 1)).requires_grad_(True)
    batch = OPS.dev(torch.arange(2).repeat_interleave(P))
    with _recorded() as rec:
        out = D(pos, dist, batch)
    assert "sg_scatter_max_fwd" in rec.names(), rec.names()
    what = "P %d ragged batch" % P
    check_forward(body, out, case.r64["out"], what)
    _check_critic_grads(body, D, out, pos, dist, case, what)
    # a leading shape [2, 3, P, .]
    lead = _critic_case(body, P, (2, 3))
    D = _critic_of(lead.sd, lead.seed)
    cpu_pos, cpu_dist = lead.x[..., :3].contiguous(), lead.x[..., 3:].contiguous()
    with torch.no_grad():
        out = D(OPS.dev(cpu_pos), OPS.dev(cpu_dist))
    assert tuple(out.shape) == (2, 3, 1)
    check_forward(body, out, lead.r64["out"], "P %d leading shape no-grad" % P)
    pos, dist = OPS.dev(cpu_pos).requires_grad_(True), OPS.dev(cpu_dist).requires_grad_(True)
    out = D(pos, dist)
    assert tuple(out.shape) == (2, 3, 1)
    what = "P %d leading shape recorded" % P
    check_forward(body, out, lead.r64["out"], what)
    _check_critic_grads(body, D, out, pos, dist, lead, what)


# ---- 10: the gradient penalty ---------------------------------------------------------------------------------------------------------
PENALTY_POINTS = (64, 1024, 1030)


def _penalty_reference(sd, x, dtype):
    """PointGANOracle.gradient_penalty at alpha = 1 (the interpolated distances are then `dist` itself, bit for bit) -> (value,
    parameter gradients)."""
    o = O.PointGANOracle({"unused": torch.zeros(1, dtype=dtype)}, {k: v.to(dtype) for k, v in sd.items()})
    pos, dist = x[..., :3].to(dtype), x[..., 3:].to(dtype)
    gp = o.gradient_penalty(pos, dist.clone(), torch.zeros_like(dist), torch.ones(x.shape[0], 1, 1, dtype=dtype))
    gp.backward()
    return gp.detach(), {k: v.grad for k, v in o.D.items()}


def body_gradient_penalty(P):
    """The critic-side penalty of PointGANOracle.critic_step — gradient of the output with respect to dist, gp_weight * ((|g| - 1)^2).mean(),
    backward to the parameters — on the dense and on the sparse branch of PointNet.forward."""
    body = "10 gradient penalty"
    case = _critic_case(body, P, (2,))
    (v32, g32), (v64, g64) = _penalty_reference(case.sd, case.x, torch.float32), _penalty_reference(case.sd, case.x, torch.float64)
    for branch, least in (("dense", 10 ** 9), ("sparse", 0)):
        D = _critic_of(case.sd, case.seed)
        D.SPARSE_MIN_POINTS = least
        pos, dist = OPS.dev(case.x[..., :3].contiguous()), OPS.dev(case.x[..., 3:].contiguous()).requires_grad_(True)
        with _recorded() as rec:
            out = D(pos, dist)
        assert ("sg_rowdot" in rec.names()) == (branch == "sparse"), "%s: %s" % (branch, rec.names())
        (grad,) = torch.autograd.grad(out, dist, torch.ones_like(out), create_graph=True)
        gp = 10.0 * ((grad.reshape(grad.shape[0], -1).norm(dim=-1, p=2) - 1).pow(2).mean())
        what = "P %d %s" % (P, branch)
        check(body, gp.reshape(1), v32.reshape(1), v64.reshape(1), what + " value")
        gp.backward()
        for k, p in D.named_parameters():
            if g64[k] is None:       # (the last bias: the penalty does not depend on it)
                assert p.grad is None or not bool(p.grad.ne(0).any()), what + ": a gradient for " + k
                continue
            check(body, p.grad, g32[k], g64[k], "%s grad %s" % (what, k))
