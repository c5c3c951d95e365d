"""Case table, float64 references and test bodies for the autograd layer of shapegan_amd/ops.py: every torch.autograd.Function
whose backward chooses between kernels, branch by branch, against float64 autograd of the plain torch composition
(tests/test_gpu_autograd.py; re-run on the twin by tests/test_cpu_twin.py).  Pure Python: nothing here is a test by itself.

One case = an `ops` callable, the float64 composition of the same operation, seeded inputs, the names of its differentiable
inputs.  body(name, order, layout, monkeypatch) runs it for EVERY non-empty subset of the differentiable inputs:

    order "first"   torch.autograd.grad((y * r).sum(), subset): grad mode is off inside backward, the raw-kernel branches run
    order "lib"     the case's parameters live in an optim.RMSprop / optim.Adam flat buffer, the subset requires grad, the
                    operation is applied once, then TWICE in one graph (two data inputs, as the critic sees real and fake) and
                    lib.backward runs.  Once: p.grad must be the view of its flat slice.  Twice: p.grad must hold the sum of
                    both contributions (the engine adds them before AccumulateGrad sees either, so p.grad is then an ordinary
                    tensor) and _Flat.adopt_grads() must bring that sum into the slice.  Both: a parameter outside the subset
                    keeps p.grad None and its slice keeps the sentinel written before
    order "second"  h = grad((y * r).sum(), subset, create_graph=True), then grad(sum h^2, subset): the gradient penalty's
                    shape.  h is checked too (the create_graph branches of every backward).  Where the reference has no path
                    (None, zeros, or sum h^2 without a graph) the library may return None, zeros or a tensor without a graph,
                    never a non-zero value.  @once_differentiable Functions must RAISE in the second grad.

    layout "fresh"     the engine hands backward a new contiguous gradient:        (y * r).sum()
    layout "expand"    a stride-0 expand over dim 0 (SumBackward's own output):    (y.sum(0) * r0).sum()
                       (BatchNorm1d: over dim 1 — the sum over the batch of a normalised column is a constant)
    layout "permuted"  a transposed view (TransposeBackward's output):             (y.transpose(0, -1) * r').sum()
                       (1-D y: the strided column that the backward of torch.stack([y, const], 1) narrows out)
A hook on y asserts that the gradient really arrives in that layout.

Kinks.  LeakyReLU / ReLU derivatives jump at 0 and two correct fp32 implementations may fall on different sides.  The float64
pre-activation z is computed; wherever |z| < KINK * rms(z) the probe is zeroed (layout "expand": the whole column over dim 0 that
holds such an element), which removes the element from both orders.  At most MAX_DROPPED of a case's elements may go this way —
asserted, the seeds below were chosen for it; where y is not element-wise in z (ConvHead) no element may be that close at all.

Which branch ran is asserted from the host side: the raw entries in TRACKED are wrapped for the duration of the backward passes and
each case names the set it expects for (subset, order, on the device or not).

Tolerance: OPS.close at RTOL = 1e-4 of the reference's mean magnitude, against the float64 result cast to fp32, both orders.
Every check prints `[autograd] family | case | order | layout | subset | what | max |got - ref| / max |ref|` before it asserts.
No case needed more than that: the largest error seen, over every case, order and layout, is 2.0e-6 of the reference's maximum on
the twin and 4.9e-6 on an MI355X (both ConvHead applied twice in one graph; everything else stays below 1.7e-6)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_ops as OPS

NONE, LEAKY, RELU, TANH, SIGMOID = 0, 1, 2, 3, 4
ACT_NAMES = {NONE: "none", LEAKY: "leaky", RELU: "relu", TANH: "tanh", SIGMOID: "sigmoid"}
SLOPE = 0.2
KINK = 1e-4
MAX_DROPPED = 0.01
SENTINEL = 7.0
LAYOUTS = ("fresh", "expand", "permuted")
ORDERS = ("first", "lib", "second")

FUSED_RAW = ("conv_wgrad_act_raw", "act_bwd_rowsum_pack8_raw", "act_bwd_rowsum_raw", "conv_wgrad_prepacked_raw")
TRACKED_OPS = FUSED_RAW + ("conv_dgrad_raw", "conv_wgrad_raw", "channel_sum_raw", "colsum_tall_raw")
TRACKED_LIB = ("sg_head_dot_bwd", "sg_act_bwd_dy")
TRACKED = TRACKED_OPS + TRACKED_LIB

ONCE_ERRORS = "once_differentiable|does not require grad"
WORST = {}      # (family, order, y / d / h / g) -> largest max |got - ref| / max |ref| seen in this process


def act_ref(z, act):
    if act == LEAKY:
        return F.leaky_relu(z, SLOPE)
    return {NONE: lambda t: t, RELU: F.relu, TANH: torch.tanh, SIGMOID: torch.sigmoid}[act](z)


def randn(*shape, scale=1.0):
    return torch.randn(*shape) * scale


class Case(object):
    """make() -> {name: fp32 CPU tensor} (plus data + "2": the second data input of order "lib"); run(ops, t) -> y;
    ref(t64) -> (y, pre-activation or None); diff: the differentiable inputs; params: those an optimizer owns in order "lib";
    direct: the parameters whose gradient backward writes straight into the flat slice; routes(subset, order, device) -> the
    expected TRACKED names: a set (exactly these) or (must include, must not include)."""

    def __init__(self, name, family, seed, make, run, ref, diff, data, params=(), direct=None, routes=None, act=NONE,
                 orders=ORDERS, layouts=LAYOUTS, once=False, after=None, expand_dim=0):
        self.name, self.family, self.seed, self.make, self.run, self.ref = name, family, seed, make, run, ref
        self.diff, self.data, self.params = tuple(diff), data, tuple(params)
        self.direct = tuple(params) if direct is None else tuple(direct)
        self.routes, self.act, self.orders, self.layouts, self.once, self.after = routes, act, orders, layouts, once, after
        self.expand_dim = expand_dim      # the dimension layout "expand" sums over
        self.seed = SEEDS.get(name, seed)

    def inputs(self):
        torch.manual_seed(self.seed)
        return self.make()


CASES = {}
# seeds that replace a case's own where that one leaves float64 pre-activations in the kink band beyond the rule above (the first
# of 1000, 1001, ... for which the float64 reference alone passes the harness' assertion in every layout, for both data inputs)
SEEDS = {"convhead-24-leaky": 1000, "convhead-128-leaky": 1074, "convhead-24-relu": 1000, "convhead-128-relu": 1074,
         "convhead-24-nobh-relu": 1000, "linear-nk0-300-leaky": 1001, "linear-kn6-300-leaky": 1103, "linear-kn6-300-relu": 1103}


def add(case):
    assert case.name not in CASES, case.name
    CASES[case.name] = case


# ---- expected routes -----------------------------------------------------------------------------------------------------------
def _second(include, act, plain=()):
    """Second order: the create_graph pass must go through `include`; the pass over sum h^2 then runs with grad mode off and may
    reach the node itself again (with a real gradient through tanh / sigmoid, with materialised zeros otherwise), so the entries
    of its plain route `plain` are allowed; no other fused entry is."""
    smooth = act in (TANH, SIGMOID)
    return (set(include) | ({"sg_act_bwd_dy"} if smooth else set()),
            (set(FUSED_RAW) | {"sg_head_dot_bwd"} | (set() if smooth else {"sg_act_bwd_dy"})) - set(plain))


def conv_fwd_routes(act, has_b, full, Co, O, fused=False, image=False):
    """ConvFwd.backward.  full: the weight has exactly x's channels; fused / image: what sg_conv3d_k4s2p1_wgrad_act_eligible /
    sg_conv3d_k4s2p1_wgrad_dy_image answer for the case's shape (both are host code and were asked when the case was written)."""
    def routes(subset, order, device):
        nx, nw, want_b = "x" in subset, "w" in subset, has_b and "b" in subset
        if order == "second":
            return _second((["conv_dgrad_raw"] if nx else []) + (["conv_wgrad_raw"] if nw else [])
                           + (["channel_sum_raw"] if want_b else []), act, routes(subset, "first", device))
        if act != NONE and want_b and nw and not nx and full and fused:
            return {"conv_wgrad_act_raw"}
        s = set()
        img = act in (LEAKY, RELU) and want_b and nw and O == 8 and full and Co % 128 == 0 and device and image
        rowsum = not img and act != NONE and want_b and O ** 3 >= 512
        if img:
            s |= {"act_bwd_rowsum_pack8_raw", "conv_wgrad_prepacked_raw"}
        if rowsum:
            s.add("act_bwd_rowsum_raw")
        if nx:
            s.add("conv_dgrad_raw")
        if nw and not img:
            s.add("conv_wgrad_raw")
        if want_b and not img and not rowsum:
            s.add("channel_sum_raw")
        return s
    return routes


def conv_dgrad_routes(act, has_b, O):
    """ConvDgrad.backward; O: the extent of its OUTPUT grid."""
    def routes(subset, order, device):
        nw, want_b = "w" in subset, has_b and "b" in subset
        if order == "second":
            return _second((["conv_wgrad_raw"] if nw else []) + (["channel_sum_raw"] if want_b else []), act,
                           routes(subset, "first", device))
        s = set()
        rowsum = act != NONE and want_b and O ** 3 >= 512
        if rowsum:
            s.add("act_bwd_rowsum_raw")
        if nw:
            s.add("conv_wgrad_raw")
        if want_b and not rowsum:
            s.add("channel_sum_raw")
        return s
    return routes


def conv_wgrad_routes(subset, order, device):
    if order == "second":
        return _second(["conv_dgrad_raw"] if "x" in subset else [], NONE)
    return {"conv_dgrad_raw"} if "x" in subset else set()


def conv_head_routes(act, has_b, image=False):
    def routes(subset, order, device):
        nx, nw, need_b = "x" in subset, "w" in subset, has_b and "b" in subset
        if order == "second":
            return _second((["conv_dgrad_raw"] if nx else []) + (["conv_wgrad_raw"] if nw else [])
                           + (["channel_sum_raw"] if need_b else []), act, routes(subset, "first", device))
        s = {"sg_head_dot_bwd"}
        if nx:
            s.add("conv_dgrad_raw")
        if nw:
            s.add("conv_wgrad_prepacked_raw" if (image and device) else "conv_wgrad_raw")
        return s
    return routes


def linear_routes(act, has_b, rows):
    def routes(subset, order, device):
        s = {"colsum_tall_raw"} if (has_b and "b" in subset and rows > 256) else set()
        if order == "second":
            return (s | ({"sg_act_bwd_dy"} if act in (TANH, SIGMOID) else set()),
                    (set(TRACKED) - {"colsum_tall_raw", "sg_act_bwd_dy"}) | (set() if act in (TANH, SIGMOID) else {"sg_act_bwd_dy"})
                    | (set() if s else {"colsum_tall_raw"}))
        return s
    return routes


def act_routes(act):
    def routes(subset, order, device):
        return {"sg_act_bwd_dy"} if (order == "second" and act in (TANH, SIGMOID)) else set()
    return routes


def no_routes(subset, order, device):
    return set()


# ---- Act / ActBwd --------------------------------------------------------------------------------------------------------------
def _act_cases():
    for act in (LEAKY, RELU, TANH, SIGMOID):
        add(Case("act-%s" % ACT_NAMES[act], "Act", 11 + act,
                 make=lambda: {"x": randn(11), "x2": randn(11)},
                 run=lambda ops, t, act=act: ops.Act.apply(t["x"], act, SLOPE),
                 ref=lambda t, act=act: (act_ref(t["x"], act), t["x"] if act in (LEAKY, RELU) else None),
                 diff=("x",), data="x", routes=act_routes(act), act=act, orders=("first", "second")))

        # ActBwd applied directly with a column sum behind it: the FIRST-order gradient w.r.t. y is sg_act_bwd_dy with the
        # stride-0 expand of ColSum.backward as its ggx (what a bias-only penalty delivers at second order).  First order only:
        # that term comes from a raw kernel and is not differentiated again (it would be the THIRD order of the activation)
        def make(act=act):
            z = randn(6, 5)
            return {"y": act_ref(z, act), "y2": act_ref(randn(6, 5), act), "dy": randn(6, 5)}

        def ref(t, act=act):
            y, dy = t["y"], t["dy"]
            d = {LEAKY: lambda: torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE)),
                 RELU: lambda: (y > 0).to(y.dtype), TANH: lambda: 1 - y * y, SIGMOID: lambda: y * (1 - y)}[act]()
            return (dy * d).sum(0), None

        def routes(subset, order, device, act=act):
            smooth = act in (TANH, SIGMOID)
            if order == "second":
                return ({"sg_act_bwd_dy"} if smooth else set(), set(TRACKED_OPS) | (set() if smooth else {"sg_act_bwd_dy"}))
            return {"sg_act_bwd_dy"} if (smooth and "y" in subset) else set()
        add(Case("actbwd-colsum-%s" % ACT_NAMES[act], "ActBwd", 21 + act, make=make,
                 run=lambda ops, t, act=act: ops.ColSum.apply(ops.ActBwd.apply(t["y"], t["dy"], act, SLOPE)),
                 ref=ref, diff=("y", "dy") if act in (TANH, SIGMOID) else ("dy",), data="y", routes=routes, act=act,
                 orders=("first",)))


# ---- ConvFwd -------------------------------------------------------------------------------------------------------------------
def _conv_fwd_ref(act, has_b=True):
    def ref(t):
        x, w = t["x"], t["w"]
        z = F.conv3d(x, w[:, :x.shape[1]], t["b"] if has_b else None, stride=2, padding=1)
        return act_ref(z, act), z if act in (LEAKY, RELU) else None
    return ref


def _conv_fwd_case(name, seed, N, Cx, Ct, Co, R, act, has_b=True, diff=("x", "w", "b"), orders=ORDERS, layouts=LAYOUTS,
                   fused=False, image=False):
    def make():
        d = {"x": randn(N, Cx, R, R, R), "x2": randn(N, Cx, R, R, R), "w": randn(Co, Ct, 4, 4, 4, scale=(Cx * 64) ** -0.5)}
        if has_b:
            d["b"] = randn(Co, scale=0.3)
        return d
    diff = tuple(k for k in diff if has_b or k != "b")
    add(Case(name, "ConvFwd", seed, make,
             run=lambda ops, t: ops.conv3d_k4s2p1(t["x"], t["w"], t.get("b"), act, SLOPE),
             ref=_conv_fwd_ref(act, has_b), diff=diff, data="x", params=tuple(k for k in ("w", "b") if has_b or k != "b"),
             routes=conv_fwd_routes(act, has_b, Cx == Ct, Co, R // 2, fused, image), act=act, orders=orders, layouts=layouts))


def _conv_fwd_cases():
    # (a) the fused weight-gradient + activation-backward route: N * O^3 = 65536 is its eligibility floor; x needs no gradient
    for act in (LEAKY, RELU):
        _conv_fwd_case("convfwd-a-fused-%s" % ACT_NAMES[act], 101 + act, 16, 1, 1, 8, 32, act, diff=("w", "b"),
                       orders=("first", "lib"), fused=True)
    # (b) output 8^3, Cout = 128, N x Cin = 24 x 15: among the smallest batches sg_conv3d_k4s2p1_wgrad_dy_image accepts (it wants
    # 384 tiles: N * Cin >= 320 at this grid).  The pack8 route on the device, act_bwd_rowsum_raw on the twin.  LeakyReLU and ReLU
    # lie on the same side of every condition of that route: LeakyReLU in every layout, ReLU in the fresh one.
    _conv_fwd_case("convfwd-b-pack8-leaky", 111, 24, 15, 15, 128, 16, LEAKY, diff=("w", "b"), orders=("first", "lib"), image=True)
    _conv_fwd_case("convfwd-b-pack8-relu", 112, 24, 15, 15, 128, 16, RELU, diff=("w", "b"), orders=("first",), layouts=("fresh",),
                   image=True)
    for act in (NONE, LEAKY, RELU, TANH, SIGMOID):
        a = ACT_NAMES[act]
        # (c) output 8^3, Cout = 5: act_bwd_rowsum_raw; (d) output 4^3: the ActBwd route; (f) every activation on both
        _conv_fwd_case("convfwd-c-8-%s" % a, 120 + act, 2, 3, 3, 5, 16, act)
        _conv_fwd_case("convfwd-d-4-%s" % a, 130 + act, 2, 3, 3, 5, 8, act)
    # (e) without a bias (the frozen bias is the subsets of (c) / (d) that leave b out)
    _conv_fwd_case("convfwd-e-8-nobias-leaky", 141, 2, 3, 3, 5, 16, LEAKY, has_b=False)
    _conv_fwd_case("convfwd-e-4-nobias-tanh", 142, 2, 3, 3, 5, 8, TANH, has_b=False)
    # (g) a weight with more input channels than x (progressive growing: w[:, :Cx])
    _conv_fwd_case("convfwd-g-slice-8-leaky", 151, 2, 2, 4, 5, 16, LEAKY)
    _conv_fwd_case("convfwd-g-slice-4-sigmoid", 152, 2, 2, 4, 5, 8, SIGMOID)


# ---- ConvDgrad -----------------------------------------------------------------------------------------------------------------
def _conv_dgrad_cases():
    def case(name, seed, N, Ci, Co, cin, R, act):
        # x [N, Ci, R^3] -> [N, cin, (2R)^3] with w [Ci, Co, 4, 4, 4] (nn.ConvTranspose3d layout), cin <= Co
        def make():
            return {"x": randn(N, Ci, R, R, R), "x2": randn(N, Ci, R, R, R), "w": randn(Ci, Co, 4, 4, 4, scale=(Ci * 8) ** -0.5),
                    "b": randn(cin, scale=0.3)}

        def run(ops, t):
            if cin == Co:
                return ops.conv_transpose3d_k4s2p1(t["x"], t["w"], t["b"], act, SLOPE)
            return ops.ConvDgrad.apply(t["x"], t["w"], t["b"], cin, act, SLOPE, False)

        def ref(t):
            z = F.conv_transpose3d(t["x"], t["w"][:, :cin], t["b"], stride=2, padding=1)
            return act_ref(z, act), z if act in (LEAKY, RELU) else None
        add(Case(name, "ConvDgrad", seed, make, run, ref, diff=("x", "w", "b"), data="x", params=("w", "b"),
                 routes=conv_dgrad_routes(act, True, 2 * R), act=act))
    for act in (NONE, LEAKY, RELU, TANH, SIGMOID):
        a = ACT_NAMES[act]
        case("convdgrad-8-%s" % a, 200 + act, 2, 4, 3, 3, 4, act)
        case("convdgrad-4-%s" % a, 210 + act, 2, 4, 3, 3, 2, act)
    case("convdgrad-8-cin-leaky", 221, 2, 4, 5, 3, 4, LEAKY)
    case("convdgrad-4-cin-tanh", 222, 2, 4, 5, 3, 2, TANH)


# ---- ConvWgrad -----------------------------------------------------------------------------------------------------------------
def _conv_wgrad_cases():
    def case(name, seed, N, Cx, ct, Co, O):
        def make():
            return {"dy": randn(N, Co, O, O, O), "dy2": randn(N, Co, O, O, O), "x": randn(N, Cx, 2 * O, 2 * O, 2 * O)}

        def ref(t):
            w0 = torch.zeros(Co, Cx, 4, 4, 4, dtype=t["x"].dtype, requires_grad=True)
            (dw,) = torch.autograd.grad(F.conv3d(t["x"], w0, None, stride=2, padding=1), w0, t["dy"], create_graph=True)
            if ct > Cx:
                dw = torch.cat([dw, torch.zeros(Co, ct - Cx, 4, 4, 4, dtype=dw.dtype)], 1)
            return dw, None
        add(Case(name, "ConvWgrad", seed, make, run=lambda ops, t: ops.ConvWgrad.apply(t["dy"], t["x"], ct), ref=ref,
                 diff=("dy", "x"), data="dy", routes=conv_wgrad_routes, orders=("first", "second")))
    case("convwgrad-4", 301, 2, 3, 3, 5, 4)
    case("convwgrad-2-slice", 302, 3, 2, 4, 5, 2)


# ---- ConvHead ------------------------------------------------------------------------------------------------------------------
def _conv_head_cases():
    def case(name, seed, N, Cx, C, act, has_b=True, has_bh=True, image=False, orders=ORDERS, layouts=LAYOUTS, diff=None):
        def make():
            d = {"x": randn(N, Cx, 8, 8, 8), "x2": randn(N, Cx, 8, 8, 8), "w": randn(C, Cx, 4, 4, 4, scale=(Cx * 64) ** -0.5),
                 "wh": randn(1, C, 4, 4, 4, scale=(C * 64) ** -0.5)}
            if has_b:
                d["b"] = randn(C, scale=0.3)
            if has_bh:
                d["bh"] = randn(1)
            return d

        def ref(t):
            z = F.conv3d(t["x"], t["w"], t.get("b"), stride=2, padding=1)
            y = (act_ref(z, act).reshape(N, -1) * t["wh"].reshape(1, -1)).sum(1)
            return (y + t["bh"]) if has_bh else y, z if act in (LEAKY, RELU) else None
        names = tuple(k for k in ("x", "w", "b", "wh", "bh") if (has_b or k != "b") and (has_bh or k != "bh"))
        add(Case(name, "ConvHead", seed, make,
                 run=lambda ops, t: ops.conv_head(t["x"], t["w"], t.get("b"), act, SLOPE, t["wh"], t.get("bh")),
                 ref=ref, diff=diff or names, data="x", params=names[1:], routes=conv_head_routes(act, has_b, image), act=act,
                 orders=orders, layouts=layouts))
    for act in (NONE, LEAKY, RELU):
        a = ACT_NAMES[act]
        case("convhead-24-%s" % a, 400 + act, 3, 2, 24, act)
        # C = 128: the head asks sg_conv3d_k4s2p1_wgrad_dy_image for an image; at x [3, 2, 8^3] the planner declines (it wants
        # 384 tiles, N * Cin >= 3008 on the 4^3 grid), so sg_head_dot_bwd is followed by the plain weight gradient
        case("convhead-128-%s" % a, 410 + act, 3, 2, 128, act)
    case("convhead-24-nob-leaky", 421, 3, 2, 24, LEAKY, has_b=False)
    case("convhead-24-nobh-relu", 422, 3, 2, 24, RELU, has_bh=False)
    # the image route of the head (the device only): N x Cin = 16 x 191 is at the planner's floor.  First order, fresh layout,
    # the convolution's own parameters only (this size costs the twin seconds per subset); no activation: y sums over z, so a
    # kink element cannot be masked, and 131072 pre-activations always hold some.
    case("convhead-128-image-none", 431, 16, 191, 128, NONE, image=True, orders=("first",), layouts=("fresh",), diff=("w", "b"))


# ---- Gemm / LinearAct / ColSum / ChannelSum --------------------------------------------------------------------------------------
def _gemm_cases():
    M, K, N = 6, 7, 10
    for ta in (False, True):
        for tb in (False, True):
            def make(ta=ta, tb=tb):
                sa, sb = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
                return {"a": randn(*sa), "a2": randn(*sa), "b": randn(*sb)}

            def ref(t, ta=ta, tb=tb):
                return (t["a"].t() if ta else t["a"]) @ (t["b"].t() if tb else t["b"]), None
            add(Case("gemm-%s%s" % ("t" if ta else "n", "t" if tb else "n"), "Gemm", 500 + 2 * ta + tb, make,
                     run=lambda ops, t, ta=ta, tb=tb: ops.Gemm.apply(t["a"], t["b"], ta, tb), ref=ref, diff=("a", "b"), data="a",
                     routes=no_routes, orders=("first", "second")))


def _linear_cases():
    for w_kn, shift in ((False, 0), (True, 6)):
        for rows in (3, 300):
            for act in (NONE, LEAKY, RELU, TANH, SIGMOID):
                def make(w_kn=w_kn, rows=rows):
                    if w_kn:      # the 1^3 -> 4^3 ConvTranspose of model/stack.py: x [rows, 5], w [5, 2 * 64], b [2]
                        return {"x": randn(rows, 5), "x2": randn(rows, 5), "w": randn(5, 128, scale=0.4), "b": randn(2, scale=0.3)}
                    return {"x": randn(rows, 5), "x2": randn(rows, 5), "w": randn(7, 5, scale=0.4), "b": randn(7, scale=0.3)}

                def ref(t, w_kn=w_kn, shift=shift, act=act):
                    z = t["x"] @ (t["w"] if w_kn else t["w"].t()) + t["b"].repeat_interleave(1 << shift)
                    return act_ref(z, act), z if act in (LEAKY, RELU) else None
                add(Case("linear-%s-%d-%s" % ("kn6" if w_kn else "nk0", rows, ACT_NAMES[act]), "LinearAct",
                         600 + 100 * w_kn + 10 * (rows > 3) + act, make,
                         run=lambda ops, t, w_kn=w_kn, shift=shift, act=act: ops.LinearAct.apply(t["x"], t["w"], t["b"], act, SLOPE,
                                                                                                 w_kn, shift),
                         ref=ref, diff=("x", "w", "b"), data="x", params=("w", "b"), routes=linear_routes(act, True, rows), act=act))


def _sum_cases():
    # the sums alone (their backward is an expand: there is no second-order path), and behind a tanh, whose backward the expand feeds
    for rows in (3, 300):
        add(Case("colsum-%d" % rows, "ColSum", 800 + rows, make=lambda rows=rows: {"g": randn(rows, 6), "g2": randn(rows, 6)},
                 run=lambda ops, t: ops.ColSum.apply(t["g"]), ref=lambda t: (t["g"].sum(0), None), diff=("g",), data="g",
                 routes=no_routes, orders=("first", "second")))
        add(Case("colsum-%d-tanh" % rows, "ColSum", 810 + rows, make=lambda rows=rows: {"g": randn(rows, 6), "g2": randn(rows, 6)},
                 run=lambda ops, t: ops.ColSum.apply(ops.Act.apply(t["g"], TANH, 0.0)),
                 ref=lambda t: (torch.tanh(t["g"]).sum(0), None), diff=("g",), data="g", routes=act_routes(TANH), act=TANH,
                 orders=("first", "second")))
    for shape in ((3, 4, 2, 2, 2), (5, 4)):
        tag = "x".join(str(s) for s in shape)
        add(Case("channelsum-%s" % tag, "ChannelSum", 820 + len(shape), make=lambda shape=shape: {"g": randn(*shape), "g2": randn(*shape)},
                 run=lambda ops, t: ops.ChannelSum.apply(t["g"]),
                 ref=lambda t: (t["g"].transpose(0, 1).reshape(t["g"].shape[1], -1).sum(1), None), diff=("g",), data="g",
                 routes=no_routes, orders=("first", "second")))
        add(Case("channelsum-%s-sigmoid" % tag, "ChannelSum", 830 + len(shape),
                 make=lambda shape=shape: {"g": randn(*shape), "g2": randn(*shape)},
                 run=lambda ops, t: ops.ChannelSum.apply(ops.Act.apply(t["g"], SIGMOID, 0.0)),
                 ref=lambda t: (torch.sigmoid(t["g"]).transpose(0, 1).reshape(t["g"].shape[1], -1).sum(1), None), diff=("g",),
                 data="g", routes=act_routes(SIGMOID), act=SIGMOID, orders=("first", "second")))


# ---- BatchNormAct --------------------------------------------------------------------------------------------------------------
EPS, MOMENTUM = 1e-5, 0.1


def _bn_cases():
    for training in (True, False):
        for shape in ((4, 3, 2, 2, 2), (4, 3)):
            for act in (NONE, LEAKY, RELU, TANH, SIGMOID):
                def make(shape=shape):
                    C = shape[1]
                    return {"x": randn(*shape) * 1.5 + 0.3, "x2": randn(*shape), "gamma": torch.rand(C) + 0.5, "beta": randn(C, scale=0.5),
                            "rm": randn(C, scale=0.2), "rv": torch.rand(C) + 0.5, "nbt": torch.tensor(3, dtype=torch.int64)}

                def run(ops, t, training=training, act=act):
                    return ops.BatchNormAct.apply(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"], t["nbt"] if training else None,
                                                  training, EPS, MOMENTUM, act, SLOPE)

                def ref(t, training=training, act=act):
                    z = F.batch_norm(t["x"], t["rm"], t["rv"], t["gamma"], t["beta"], training, MOMENTUM, EPS)
                    if training:
                        t["nbt"] += 1      # (nn.BatchNorm's own bookkeeping around F.batch_norm)
                    return act_ref(z, act), z if act in (LEAKY, RELU) else None

                def after(got, want, what):
                    for k in ("rm", "rv"):
                        check(got[k], want[k], "BatchNormAct", what + " | " + k)
                    assert int(got["nbt"]) == int(want["nbt"]), what + ": num_batches_tracked"
                add(Case("bn-%s-%dd-%s" % ("train" if training else "eval", len(shape), ACT_NAMES[act]), "BatchNormAct",
                         900 + 40 * training + 10 * len(shape) + act, make, run, ref, diff=("x", "gamma", "beta"), data="x",
                         params=("gamma", "beta"), routes=no_routes, act=act, once=True, after=after,
                         # (training BatchNorm1d: the sum over the batch of a normalised column is the constant N * beta)
                         expand_dim=1 if len(shape) == 2 else 0))


_act_cases()
_conv_fwd_cases()
_conv_dgrad_cases()
_conv_wgrad_cases()
_conv_head_cases()
_gemm_cases()
_linear_cases()
_sum_cases()
_bn_cases()

PARAMS = [(c.name, order, layout) for c in CASES.values() for order in c.orders for layout in c.layouts]


# ---- the harness ---------------------------------------------------------------------------------------------------------------
def check(got, ref, family, what):
    """got (None = no gradient) against the float64-made ref (None = no path): OPS.close at RTOL; where the reference is zero
    the library must be exactly zero."""
    ref = None if ref is None else ref.detach()
    if ref is None or float(ref.abs().max()) == 0.0:
        assert got is None or float(got.detach().abs().max()) == 0.0, what + ": a non-zero value where the reference has no path"
        print("[autograd] %s | %s | no path" % (family, what))
        return
    assert got is not None, what + ": no gradient where the reference has one"
    ref32 = ref.detach().float().cpu()
    got = got.detach().float().cpu()
    assert got.shape == ref32.shape, what + ": shape %s, expected %s" % (tuple(got.shape), tuple(ref32.shape))
    err = float((got.double() - ref.detach().double().cpu()).abs().max()) / float(ref.abs().max())
    key = (family, what.split(" | ")[1], what.split(" | ")[-1][0])      # order; y / d / h / g
    WORST[key] = max(WORST.get(key, 0.0), err)
    print("[autograd] %s | %s | %.3e" % (family, what, err))
    OPS.close(got, ref32, what=what)


def subsets(names):
    return [s for n in range(1, len(names) + 1) for s in itertools.combinations(names, n)]


def _probes(case, y, pre, layout):
    """The probe of each layout as a float64 CPU tensor, with the kink elements of y taken out; asserts the dropped fraction."""
    r = torch.randn(y.shape).double()      # (fp32 values: both sides multiply by the same numbers)
    keep = torch.ones(y.shape, dtype=torch.bool)
    if pre is not None:
        near = pre.detach().abs() < KINK * float(pre.detach().pow(2).mean().sqrt())
        if near.shape == y.shape:
            keep = ~near
        else:
            assert not bool(near.any()), "%s: a pre-activation within the kink band (choose another seed)" % case.name
    if layout == "fresh":
        probe = r * keep
    elif layout == "expand":
        if y.dim() == 1:
            probe, keep = r[0].clone(), keep & bool(keep.all())
        else:
            d = case.expand_dim
            col = keep.all(d)
            probe, keep = r.select(d, 0) * col, col.unsqueeze(d).expand(y.shape)
    else:
        probe = torch.stack([r * keep, torch.randn(y.shape).double()], 1) if y.dim() == 1 \
            else (r * keep).transpose(0, -1).contiguous()
    dropped = 1.0 - float(keep.double().mean())
    assert dropped <= MAX_DROPPED, "%s: %.2f%% of the elements lie in the kink band" % (case.name, 100 * dropped)
    return probe


def _loss(y, probe, layout, expand_dim=0):
    if layout == "fresh":
        return (y * probe).sum()
    if layout == "expand":
        return y.sum() * probe if y.dim() == 1 else (y.sum(expand_dim) * probe).sum()
    if y.dim() == 1:
        return (torch.stack([y, torch.zeros_like(y)], 1) * probe).sum()
    return (y.transpose(0, -1) * probe).sum()


def _f64(t):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in t.items()}


def _second_order(loss, leaves, once=False):
    """(h, grad of sum h^2) with None where there is no gradient / no path."""
    h = torch.autograd.grad(loss, leaves, create_graph=True, allow_unused=True)
    s = sum((hi * hi).sum() for hi in h if hi is not None)
    if once:      # (h comes back without a graph when the incoming gradient has none, with a node that raises otherwise)
        with pytest.raises(RuntimeError, match=ONCE_ERRORS):
            torch.autograd.grad(s, leaves, allow_unused=True)
        return h, None
    if not (torch.is_tensor(s) and s.requires_grad):
        return h, [None] * len(leaves)
    return h, torch.autograd.grad(s, leaves, allow_unused=True)


class _Recorder(object):
    """Wraps the TRACKED entries; names are recorded only while `on`."""

    def __init__(self, monkeypatch):
        from shapegan_amd import ops
        self.on, self.seen = False, set()
        lib = ops._lib()
        for owner, names in ((ops, TRACKED_OPS), (lib, TRACKED_LIB)):
            for name in names:
                monkeypatch.setattr(owner, name, self._wrap(name, getattr(owner, name)))

    def _wrap(self, name, real):
        def wrapped(*a, **k):
            if self.on:
                self.seen.add(name)
            return real(*a, **k)
        return wrapped

    def start(self):
        self.on, self.seen = True, set()

    def stop(self, case, subset, order, device, what):
        self.on = False
        want = case.routes(subset, order, device)
        if isinstance(want, tuple):
            assert want[0] <= self.seen and not (want[1] & self.seen), "%s: entries called %s, expected to include %s and none of %s" \
                % (what, sorted(self.seen), sorted(want[0]), sorted(want[1] & self.seen))
        else:
            assert self.seen == want, "%s: entries called %s, expected %s" % (what, sorted(self.seen), sorted(want))


def body(name, order, layout, monkeypatch):
    case = CASES[name]
    base = case.inputs()
    rec = _Recorder(monkeypatch)
    for subset in subsets(case.diff):
        if order == "lib":
            # once alone (p.grad must BE the flat slice), once twice in one graph (the engine sums the two contributions before
            # AccumulateGrad sees them: p.grad holds the sum; adopt_grads() puts it back into the slice)
            _run(case, base, rec, subset, order, layout, (case.data,))
            _run(case, base, rec, subset, order, layout, (case.data, case.data + "2"))
        else:
            _run(case, base, rec, subset, order, layout, (case.data,))


def _run(case, base, rec, subset, order, layout, uses):
    from shapegan_amd import ops, optim
    import shapegan_amd.lib as L
    twice = len(uses) == 2
    what = "%s | %s | %s | %s" % (case.name, order + ("2" if twice else ""), layout, "+".join(subset))

    def forward(t, run):
        """[(y, pre)] of the one or two applications."""
        out = []
        for d in uses:
            td = dict(t)
            td[case.data] = t[d]
            res = run(td)
            out.append(res if isinstance(res, tuple) else (res, None))
        return out

    def leaves_of(t):
        for k in subset:
            t[k].requires_grad_(True)
            if twice and k == case.data:
                t[k + "2"].requires_grad_(True)
        return [t[k] for k in subset]

    # ---- float64 reference
    t64 = _f64(base)
    leaves64 = leaves_of(t64)
    torch.manual_seed(case.seed + 7)
    outs = forward(t64, case.ref)
    probes = [_probes(case, y, pre, layout) for y, pre in outs]
    loss64 = sum(_loss(y, p, layout, case.expand_dim) for (y, _), p in zip(outs, probes))
    # ---- the library
    t = {k: v.cuda() for k, v in base.items()}
    device = t[case.data].is_cuda
    leaves = leaves_of(t)
    opt = None
    if order == "lib" and case.params:
        opt = (optim.RMSprop if len(subset) % 2 else optim.Adam)([t[k] for k in case.params])
        opt.zero_grad()
        opt.flat_grad.fill_(SENTINEL)
    delivered = []
    ys = forward(t, lambda td: case.run(ops, td))
    for y, _ in ys:
        y.register_hook(lambda g: delivered.append(g is None or g.is_contiguous()))
    loss = sum(_loss(y, p.float().cuda(), layout, case.expand_dim) for (y, _), p in zip(ys, probes))
    for (y, _), (y64, _) in zip(ys, outs):
        check(y, y64, case.family, what + " | y")
    if case.after is not None:
        case.after(t, t64, what)
    rec.start()
    if order == "first":
        want = torch.autograd.grad(loss64, leaves64, allow_unused=True)
        got = torch.autograd.grad(loss, leaves, allow_unused=True)
        rec.stop(case, subset, order, device, what)
        for k, g, w in zip(subset, got, want):
            check(g, w, case.family, what + " | d" + k)
    elif order == "lib":
        loss64.backward()
        L.backward(loss)
        rec.stop(case, subset, order, device, what)
        for final in ((False, True) if (twice and opt is not None) else (False,)):
            if final:
                opt.f.adopt_grads()
            for k in subset:
                if k == case.data and twice:
                    check(t[k + "2"].grad, t64[k + "2"].grad, case.family, what + " | d" + k + "2")
                check(t[k].grad, t64[k].grad, case.family, what + " | d" + k)
            for i, k in enumerate(case.params):
                o, n = opt.f.offsets[i], t[k].numel()
                if k in subset:
                    if k in case.direct and (final or not twice):
                        assert opt.f.grad_view_ok(i), what + ": p.grad of %s is not the view of its flat slice" % k
                else:
                    assert t[k].grad is None, what + ": the frozen %s received a gradient" % k
                    if not final:      # (adopt_grads() zeroes the slice of a parameter without a gradient, by design)
                        assert bool((opt.flat_grad[o:o + n] == SENTINEL).all()), what + ": the flat slice of the frozen %s was written" % k
    else:
        h64, g64 = _second_order(loss64, leaves64)
        h, g = _second_order(loss, leaves, case.once)
        rec.stop(case, subset, order, device, what)
        for k, a, b in zip(subset, h, h64):
            check(a, b, case.family, what + " | h" + k)
        if not case.once:
            for k, a, b in zip(subset, g, g64):
                check(a, b, case.family, what + " | g" + k)
    assert len(delivered) >= len(ys), what + ": backward did not reach y"
    if layout != "fresh":      # (the first pass over the graph; a second-order pass reaches y again with other gradients)
        assert not any(delivered[:len(ys)]), what + ": the incoming gradient arrived contiguous"
    del opt


def body_sample_packed_inputs():
    """mesh.sample_packed converts float64 vertices and a non-contiguous faces view itself: the result must be bit-identical to
    the call with contiguous fp32 / int inputs (the converted copies have to live until the kernel has read them)."""
    from shapegan_amd.mesh import marching_cubes, sample_packed
    torch.manual_seed(5)
    R = 12
    ax = torch.linspace(-1, 1, R)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    grids = torch.stack([(xx ** 2 + yy ** 2 + zz ** 2).sqrt() - 0.6, (xx.abs() + yy.abs() + zz.abs()) - 0.8]).cuda()
    mb = marching_cubes(grids, 0.0)
    u = torch.rand(2, 257, 3).cuda()
    want, want_empty = sample_packed(mb.vertices, mb.faces, mb.vert_offsets, mb.tri_offsets, u)
    assert mb.faces.shape[0] > 100 and not bool(want_empty.any())
    wide = torch.zeros((mb.faces.shape[0], 2 * mb.faces.shape[1]), dtype=mb.faces.dtype, device=mb.faces.device)
    wide[:, ::2] = mb.faces
    view = wide[:, ::2]
    assert not view.is_contiguous()
    for _ in range(3):
        got, got_empty = sample_packed(mb.vertices.double(), view, mb.vert_offsets, mb.tri_offsets, u)
        assert torch.equal(got, want) and torch.equal(got_empty, want_empty)


def body_once_differentiable_losses_raise():
    """The loss Functions and LayerNormAct are @once_differentiable: a second grad through them raises, it never returns a number."""
    from shapegan_amd import ops
    torch.manual_seed(9)

    def twice(fn, *shapes):
        xs = [randn(*s).cuda().requires_grad_(True) for s in shapes]
        y = fn(*xs)
        h = torch.autograd.grad((y * torch.randn(y.shape).cuda()).sum(), xs, create_graph=True, allow_unused=True)
        s = sum((hi * hi).sum() for hi in h if hi is not None)
        with pytest.raises(RuntimeError, match=ONCE_ERRORS):
            torch.autograd.grad(s, xs, allow_unused=True)
    target = randn(3, 7, 5).cuda()
    twice(lambda o: ops.weighted_l1(o, target, 2.0), (3, 7, 5))
    twice(lambda m, lv: ops.kld(m, lv), (4, 6), (4, 6))
    twice(lambda x: ops.mean_sq(x), (5, 3))
    twice(lambda x, zb, g, b: ops.layernorm_act(x, zb, 4, g, b, 1e-5, RELU, None), (8, 6), (2, 6), (6,), (6,))
