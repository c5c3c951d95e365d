"""Case table, float64 references, bounds and test bodies for BatchNorm (K4, shapegan_amd/csrc/batchnorm.hip) in every dispatch form
(tests/test_gpu_batchnorm_forms.py; the plans the cases claim are asserted without a GPU by tests/test_batchnorm_plan_host.py; the bodies
are re-run on the twin by tests/test_cpu_twin.py).  Pure Python: nothing here is a test by itself.

Entries.  sg_bn_train_fwd, sg_bn_eval_fwd and sg_bn_bwd (train 1 and 0) through ops.BatchNormAct, sg_bn_train_fwd_grouped through
ops.bn_train_fwd_grouped_raw, sg_bn_train_stats_grouped through ops.bn_train_stats_affine.  ops allocates its outputs itself, so every
variant is ALSO run through the library entry directly ("raw") with x, dy and every output (y, save_mean, save_invstd, running_mean,
running_var, num_batches_tracked, scale, shift, dx, dgamma, dbeta) inside larger buffers whose margins hold NaN (-7 around the
counter) and with a workspace of exactly the byte count the entry asks for between two fences (gemm_forms.Workspace).  The margins
must be unchanged afterwards, a read outside x or dy shows up in the sums, and the two runs must agree bit for bit (which is also
the determinism check: same case, two runs, two workspaces).  x and dy of the ops run are views inside NaN buffers as well.

Reference.  The float64 formula written out in torch: mean, biased variance, 1 / sqrt(var + eps), the affine map, the activation;
running statistics with the unbiased variance, group after group; gradients from float64 autograd of that composition.  With one
value per channel (n == 1) torch itself raises in training; the reference is the same formula with var = 0 and running_var updated
with var itself, which is what the kernel documents.

Checks.  (a) ordinary variants: OPS.close at RTOL = 1e-4 of the reference's mean magnitude on every output.  (b) every variant,
the hard ones included: element-wise bounds built only from float64 reference quantities, u = 2^-24.

  forward   |y - y_ref| <= K_FWD u (|x scale_c| + |shift_c| + 1) L,    scale_c = gamma_c invstd_c, shift_c = beta_c - mean_c scale_c,
            L the activation's Lipschitz constant (1; 1/4 for sigmoid): the rounding of fma(x, sc, sh) with sh = beta - mean sc.  It
            grows with |mean| / std as it must, because save_mean is fp32.
  backward  dx = gamma invstd (g - mean(g) - xhat mean(g xhat)),  g = dy act'(z),  z = gamma xhat + beta.  The kernel forms xhat =
            (x - mean32) invstd32 from the fp32 mean, whose error of up to u |mean| becomes an ABSOLUTE error u |mean| invstd of
            xhat.  With I_c = 1 + |mean_c| invstd_c the magnitude that carries xhat's error therefore is
                X = |xhat| I_c + (I_c - 1)          (>= |xhat| + |mean| invstd; equal to |xhat| when the mean is 0)
            i.e. xhat inflated by I_c, plus the additive I_c - 1 for the elements near the mean, where a relative inflation vanishes
            but the error of the fp32 mean does not.  Through tanh / sigmoid the recomputed z carries the forward bound's error into
            act': with A2 = max |act''| (1 for tanh, 0.1 for sigmoid, 0 otherwise) the magnitude of g is G = |g| + |dy| A2 (|x scale_c|
            + |shift_c| + 1).  The sum of the absolute values of dx's terms then bounds it:
                |dx - dx_ref| <= K_BWD u |gamma_c| invstd_c (G + mean(G) + X mean(G X))       training
                |dx - dx_ref| <= K_BWD u |gamma_c| invstd_c G                                 eval (mean and invstd are constants)
                |dbeta - ref| <= K_BWD u sum(G),   |dgamma - ref| <= K_BWD u sum(G X)         (the same sums, not divided by n)
  statistics  where (a) does not apply: save_mean = fl(K + m) within K_FWD u (|mean| + std); save_invstd and scale within K_FWD u of
            their magnitude (fp32 sums of (x - K)^2 with K a few std from the mean); shift within K_FWD u (|beta| + |mean scale| +
            |scale| std).

Two terms of the backward bound go beyond the issue's formula, which inflates xhat by I_c and nothing else: the additive I_c - 1 in X,
and the A2 |dy| (...) term of G for tanh and sigmoid.  Both are derived above, and torch's fp32 is measured against the same bound.

(a) does not apply to the hard variants.  In the training variants with one or two values per channel (1x3x1, 2x3x1) it applies to
y and the statistics but not to dx, dgamma, dbeta: xhat is 0, or +-1 up to eps, the gradients are the remainders of terms that cancel
(dx about 1e-5 of its terms at 2x3x1), and a tolerance relative to the result says nothing; the bounds, which know the terms, hold.

K_FWD and K_BWD are not fitted to the kernels.  Over this file's final case table (122 variants, torch_fp32_ratios() below), torch's
own fp32 F.batch_norm and its autograd on the CPU reach 8.12 of the forward magnitude (9000x3x1 in training: its column sums over
9000 rows; 4.34 elsewhere) and 3.83 of the backward one (2x600x4100 in eval, dx).  4 x that, for a different and equally valid
summation order, rounded up to a power of two: K_FWD = 64, K_BWD = 16.
Every check prints `[bn-forms] shape | variant | output | max |got - ref| / bound` before it asserts.  Largest ratios of the kernels
over the table (forward: y; backward: dx, dgamma, dbeta; the statistics' bounds apply to the hard variants only):
                 y        dx       dgamma   dbeta    save_mean  save_invstd  scale    shift
    twin         0.086    0.37     0.056    0.1      0.013      0.079      0.088      0.038
    MI355X       0.068    0.37     0.056    0.1      0.013      0.079      0.088      0.036
The finding.  With the one-pass sums alone (shift K = the channel's first element, as the parent had it) the twin, which forms the
sums as the kernel does, reaches 3.0 of the y bound at 129x8x68 and 2.0 at 5x3x1721 in the hard variants (first failures): a first
element 100 or 1e3 std from the rest makes E[(x-K)^2] - E[x-K]^2 cancel 1e4- to 1e6-fold, where torch fp32 stays inside the bound.
The fix is a second pass, not another shift (csrc/batchnorm_core.h: sg_bn_shift_was_far; csrc/batchnorm.hip: bn_group_stats): when
the sums themselves show m^2 > 64 var, i.e. K more than 8 std from the mean, the finalize forms the channel's sums again around
K + m, one wave, in double, and mean and invstd come from that second pass; every other channel keeps the one-pass sums and the
parent's bits.  The threshold is measured: the one-pass invstd is off by about 0.05 (1 + m^2 / var) u, and a first element 25 std
out (below an earlier threshold of 32 std) reached 1.2 and 1.7 of the dx bound at the two hard shapes; the kind "first7" keeps the
one-pass path tested just below the threshold, where its cancellation is worst.  With the second pass a shift of 0 instead of the
first element is no longer a numerical fault (mean / std = 1e3 and 1e4 are caught by the same test of the sums and recomputed), only
a slow one; without the second pass it fails 129x8x68, 5x3x1721 and 1x3x1.

Kinks.  LeakyReLU / ReLU: dy is zeroed wherever the float64 pre-activation is within the forward bound of 0.  At most 1 % of a
variant's elements may go this way (asserted; seeds: SEEDS below; the reference alone meets it: the largest fraction over the table
is 0.78 %, in the hard variants of 129x8x68 where a channel of mean / std = 1e4 has a wide band; 0.71 % at 5x3x1721; below 0.01 %
in every ordinary variant).

Hard numerics (129x8x68 and 5x3x1721, training, forward and backward, four rotations so that every channel kind occurs at both
shapes): per channel one of mean / std = 1e3; mean / std = -1e4; a constant channel; a channel whose first element (sample 0,
position 0) lies 7 std (one pass), 100 std or 1e3 std (second pass) from the rest; values of std 1e-30; gamma = 0; gamma < 0; an
ordinary channel.

Case table: SHAPES below, (N, C, S) -> (nsplit, napply), and per shape the lengths mod 2048 of its statistics slices (all but the
last, the last): the two-groups-in-flight loop of bn_bwd_stats_kernel ends with a single-group tail in the lanes below the remainder
when that is in (0, 1024], in the lanes from remainder - 1024 on when it is in (1024, 2048), in no lane when it is 0.
"""
import torch
import torch.nn.functional as F

import test_gpu_ops as OPS
from gemm_forms import Workspace

U = 2.0 ** -24
K_FWD = 64.0
K_BWD = 16.0
MAX_DROPPED = 0.01
NONE, LEAKY, RELU, TANH, SIGMOID = 0, 1, 2, 3, 4
ACT_NAMES = {NONE: "none", LEAKY: "leaky", RELU: "relu", TANH: "tanh", SIGMOID: "sigmoid"}
SG_ERR_ARG, SG_ERR_WORKSPACE = -1, -3
NAN_BITS = 0x7FC00000
COUNTER_MARGIN = -7
WORST = {}          # "fwd" / "bwd" / "dropped" -> the largest ratio (fraction) seen in this process


def _lib():
    from shapegan_amd import ops
    return ops._lib()


# A variant is seeded by its name; where that seed leaves more than MAX_DROPPED of the float64 pre-activations in the kink band (a channel
# of mean / std = 1e4 has a band 0.08 gamma wide, and beta decides how much of the channel lies in it), by its name plus the first of
# "#1", "#2", ... for which the reference alone meets the limit.
SEEDS = {"5x3x1721 | train-leaky0.2-all-m0.1-e1e-05-hard1": "#2"}


def _seed(name):
    torch.manual_seed(sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31))


# ---- case table -----------------------------------------------------------------------------------------------------------------------
ALL_ACTS = [(NONE, 0.0), (LEAKY, 0.2), (LEAKY, 0.01), (RELU, 0.0), (TANH, 0.0), (SIGMOID, 0.0)]
TWO_ACTS = [(LEAKY, 0.2), (NONE, 0.0)]
TWO_ACTS_B = [(LEAKY, 0.01), (NONE, 0.0)]


class Shape(object):
    """x [N, C, S] with the plan it claims: (nsplit, napply), vector (float4, S % 4 == 0) or scalar, and `slices`: the lengths mod
    2048 of the statistics slices (all but the last, the last)."""

    def __init__(self, N, C, S, plan, slices, what, acts=None, hard=False, twin=True):
        self.N, self.C, self.S, self.plan, self.slices, self.what = N, C, S, tuple(plan), tuple(slices), what
        self.vector = S % 4 == 0
        self.acts = acts or (TWO_ACTS if (N + C) % 2 else TWO_ACTS_B)
        self.hard, self.twin = hard, twin
        self.id = "%dx%dx%d" % (N, C, S)

    def slice_lengths(self):
        """the statistics slices' lengths from the plan claimed (the arithmetic of sg_bn_slice)"""
        total, ns = self.N * self.S, self.plan[0]
        chunk = ((total + ns - 1) // ns + 3) & ~3
        return [min(total, (i + 1) * chunk) - i * chunk for i in range(ns)], chunk


SHAPES = [
    #     N     C      S   (nsplit, napply)  slices mod 2048
    Shape(129, 8, 68, (2, 2), (292, 288), "float4, beg = 4388 mid-sample, step > S, last slice 4384", acts=ALL_ACTS, hard=True),
    Shape(33, 16, 252, (2, 2), (64, 60), "float4, mid-sample, last slice 4156"),
    Shape(5, 3, 1721, (2, 2), (208, 205), "scalar, mid-sample", acts=ALL_ACTS, hard=True),
    Shape(3, 5, 4099, (3, 3), (4, 1), "scalar, last slice 4097"),
    Shape(9000, 3, 1, (2, 2), (404, 404), "BatchNorm1d, scalar"),
    Shape(7, 1, 37449, (63, 63), (68, 1927), "scalar, ragged last slice"),
    Shape(100, 2, 4096, (64, 100), (256, 256), "the 64 cap, napply > nsplit", acts=ALL_ACTS),
    Shape(70, 2, 4100, (64, 70), (392, 160), "the same with ragged slices"),
    Shape(2, 600, 4100, (1, 2), (8, 8), "C > 512, one stats slice, two apply slices", twin=False),
    Shape(2, 1, 8, (1, 1), (16, 16), "small end"),
    Shape(2, 3, 1, (1, 1), (2, 2), "small end, n == 2"),
    Shape(1, 3, 1, (1, 1), (1, 1), "n == 1: var = 0, running_var updated with var itself (torch raises in training)"),
    Shape(4, 24, 4096, (4, 4), (0, 0), "anchor of test_batchnorm_train_fwd_bwd: slices of whole samples"),
    Shape(3, 7, 27, (1, 1), (81, 81), "anchor of test_batchnorm_train_fwd_bwd"),
    # the two exits of the two-groups-in-flight loop with a non-empty tail: slice lengths mod 2048 in (1024, 2048) and in (0, 1024]
    Shape(11, 16, 1024, (2, 2), (1536, 1536), "float4, slices of 5632 = 2 x 2048 + 1536, beg mid-sample, step == S"),
    Shape(19, 12, 500, (2, 2), (656, 652), "float4, slices of 4752 and 4748 = 2 x 2048 + 656 / 652, mid-sample, step > S"),
    Shape(3, 4, 3400, (2, 2), (1004, 1004), "float4, slices of 5100 = 2 x 2048 + 1004, beg = 5100 mid-sample, step < S"),
]
BY_ID = {s.id: s for s in SHAPES}
assert len(BY_ID) == len(SHAPES)
TWIN_IDS = [s.id for s in SHAPES if s.twin]
HARD_IDS = [s.id for s in SHAPES if s.hard]

# grouped forms: (groups, per, C, S) -> nsplit of one group [per, C, S]
GROUPED = [(1, 33, 16, 252, 2), (2, 33, 16, 252, 2), (5, 5, 3, 1721, 2), (5, 3, 7, 27, 1), (2, 11, 16, 1024, 2),
           (64, 2, 3, 8, 1), (64, 130, 2, 64, 2)]
GROUPED_IDS = ["g%d-%dx%dx%d" % g[:4] for g in GROUPED]
GROUPED_BY_ID = dict(zip(GROUPED_IDS, GROUPED))


def variants(shape):
    """The variants of one shape: every activation of the shape in training (all of x, gamma, beta / x alone, alternating) and in
    eval (the other way round); momentum 0.1 / 1.0 and eps 1e-5 / 1e-3 alternate; one training variant without running statistics."""
    out = []
    for i, (act, slope) in enumerate(shape.acts):
        out.append(dict(training=True, act=act, slope=slope, grads="all" if i % 2 == 0 else "x", momentum=(0.1, 1.0)[i % 2],
                        eps=(1e-5, 1e-3)[i % 2], running=True))
        out.append(dict(training=False, act=act, slope=slope, grads="x" if i % 2 == 0 else "all", momentum=0.1,
                        eps=(1e-3, 1e-5)[i % 2], running=True))
    act, slope = shape.acts[0]
    out.append(dict(training=True, act=act, slope=slope, grads="all", momentum=0.1, eps=1e-5, running=False))
    if shape.hard:
        for rot in range(4):
            for act, slope in ((LEAKY, 0.2), (NONE, 0.0)):
                out.append(dict(training=True, act=act, slope=slope, grads="all", momentum=0.1, eps=1e-5, running=True, hard=rot))
    for v in out:
        v["tag"] = "%s-%s%s-%s-m%g-e%g%s%s" % ("train" if v["training"] else "eval", ACT_NAMES[v["act"]],
                                               ("%g" % v["slope"]) if v["act"] == LEAKY else "", v["grads"], v["momentum"], v["eps"],
                                               "" if v["running"] else "-norunning", "-hard%d" % v["hard"] if "hard" in v else "")
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
# (ordered so that at C = 3 no rotation holds both wide-band kinds, mean1e3 and mean-1e4: together they put 2 % of the elements in the band)
HARD_KINDS = ["first7", "constant", "mean1e3", "mean-1e4", "first100", "first1000", "tiny", "gamma0", "gammaneg", "ordinary"]


def make_inputs(shape, v, groups=1):
    """fp32 CPU tensors: x [groups * N, C, S], dy like x, gamma, beta, running_mean, running_var [C]"""
    N, C, S = groups * shape.N, shape.C, shape.S
    x = torch.randn(N, C, S) * (torch.rand(C) * 1.5 + 0.5)[None, :, None] + (torch.randn(C) * 2.0)[None, :, None]
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    if "hard" in v:
        for c in range(C):
            kind = HARD_KINDS[(c + 3 * v["hard"]) % len(HARD_KINDS)]
            r = torch.randn(N, S)
            if kind == "mean1e3":
                x[:, c] = r + 1e3
            elif kind == "mean-1e4":
                x[:, c] = r * 0.5 - 5e3
            elif kind == "constant":
                x[:, c] = 1.7
            elif kind in ("first100", "first1000", "first7"):
                x[:, c] = r
                x[0, c, 0] = {"first100": 100.0, "first1000": -1000.0, "first7": 7.0}[kind]
            elif kind == "tiny":
                x[:, c] = r * 1e-30
            elif kind == "gamma0":
                gamma[c] = 0.0
            elif kind == "gammaneg":
                gamma[c] = -gamma[c]
    dy = torch.randn(N, C, S)
    rm, rv = torch.randn(C), torch.rand(C) + 0.5
    return x, dy, gamma, beta, rm, rv


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------------
def _act64(z, act, slope):
    if act == LEAKY:
        return F.leaky_relu(z, slope)
    return {NONE: lambda t: t, RELU: torch.relu, TANH: torch.tanh, SIGMOID: torch.sigmoid}[act](z)


def _act_grad64(z, act, slope):
    if act == LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    if act == RELU:
        return (z > 0).double()
    if act == TANH:
        return 1 - torch.tanh(z) ** 2
    if act == SIGMOID:
        s = torch.sigmoid(z)
        return s * (1 - s)
    return torch.ones_like(z)


def _stats64(xd):
    """mean and biased variance per channel of xd [N, C, S] (differentiable)"""
    mean = xd.mean((0, 2))
    var = ((xd - mean[None, :, None]) ** 2).mean((0, 2))
    return mean, var


def running64(rm, rv, mean, var, n, momentum):
    unbiased = var * n / (n - 1) if n > 1 else var
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unbiased


def reference(x, dy, gamma, beta, rm, rv, v):
    """Everything in float64: outputs, gradients (autograd of the composition), the magnitudes of the bounds, and dy with the kink
    band zeroed (fp32, what both runs are given)."""
    act, slope, eps, training = v["act"], v["slope"], v["eps"], v["training"]
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    n = x.shape[0] * x.shape[2]
    if training:
        mean, var = _stats64(xd)
    else:
        mean, var = rm.double(), rv.double()
    invstd = 1 / torch.sqrt(var + eps)
    xhat = (xd - mean[None, :, None]) * invstd[None, :, None]
    z = xhat * gd[None, :, None] + bd[None, :, None]
    y = _act64(z, act, slope)
    ref = {"mean": mean.detach(), "invstd": invstd.detach(), "var": var.detach()}
    with torch.no_grad():
        sc = gd * invstd
        sh = bd - mean * sc
        ref["scale"], ref["shift"] = sc, sh
        zmag = (xd * sc[None, :, None]).abs() + sh.abs()[None, :, None] + 1
        ref["fwd_bound"] = K_FWD * U * zmag * (0.25 if act == SIGMOID else 1.0)
        dyd = dy.double()
        if act in (LEAKY, RELU):
            band = z.abs() <= K_FWD * U * zmag
            ref["dropped"] = float(band.double().mean())
            dyd = torch.where(band, torch.zeros_like(dyd), dyd)
        else:
            ref["dropped"] = 0.0
        if training and v["running"]:
            ref["rm"], ref["rv"] = running64(rm.double(), rv.double(), mean, var, n, v["momentum"])
    ref["dy"] = dyd.float()
    y.backward(dyd)
    ref["y"], ref["dx"], ref["dgamma"], ref["dbeta"] = y.detach(), xd.grad, gd.grad, bd.grad
    with torch.no_grad():
        a2 = {TANH: 1.0, SIGMOID: 0.1}.get(act, 0.0)
        infl = 1 + mean.abs() * invstd
        X = xhat.abs() * infl[None, :, None] + (infl - 1)[None, :, None]
        G = (dyd * _act_grad64(z, act, slope)).abs() + dyd.abs() * a2 * zmag
        coef = K_BWD * U * (gd.abs() * invstd)[None, :, None]
        if training:
            ref["dx_bound"] = coef * (G + G.mean((0, 2))[None, :, None] + X * (G * X).mean((0, 2))[None, :, None])
        else:
            ref["dx_bound"] = coef * G
        ref["dbeta_bound"] = K_BWD * U * G.sum((0, 2))
        ref["dgamma_bound"] = K_BWD * U * (G * X).sum((0, 2))
        std = torch.sqrt(var)
        ref["mean_bound"] = K_FWD * U * (mean.abs() + std)
        ref["invstd_bound"] = K_FWD * U * invstd
        ref["scale_bound"] = K_FWD * U * sc.abs()
        ref["shift_bound"] = K_FWD * U * (bd.abs() + (mean * sc).abs() + sc.abs() * std) + 1e-300
    for k in list(ref):
        if torch.is_tensor(ref[k]):
            ref[k] = ref[k].detach()
    return ref


# ---- guarded buffers -------------------------------------------------------------------------------------------------------------------------
class Guarded(object):
    """A tensor of `shape` inside a larger buffer: `off` elements in front (a multiple of 4 keeps the 16-byte alignment the float4
    kernels need), `tail` behind, NaN in both margins (and in the window of an output until the kernel writes it)."""

    def __init__(self, shape, values=None, off=3, tail=37):
        n = 1
        for d in shape:
            n *= d
        self.off, self.n = off, n
        buf = torch.full((off + n + tail,), float("nan"), dtype=torch.float32)
        if values is not None:
            buf[off:off + n] = values.reshape(-1)
        self.buf = buf.to(OPS.DEV)
        self.view = self.buf[off:off + n].view(shape)

    def intact(self, what):
        bits = self.buf.view(torch.int32)
        ok = bool((bits[:self.off] == NAN_BITS).all()) and bool((bits[self.off + self.n:] == NAN_BITS).all())
        assert ok, what + ": an element outside the window was written"

    def untouched(self, what):
        assert bool((self.buf.view(torch.int32) == NAN_BITS).all()), what + ": a refused call wrote to an output"

    def get(self, what):
        self.intact(what)
        return self.view.clone().cpu()


class Counter(object):
    """num_batches_tracked between two sentinels"""

    def __init__(self, start=3):
        self.buf = torch.tensor([COUNTER_MARGIN, start, COUNTER_MARGIN], dtype=torch.int64).to(OPS.DEV)
        self.view = self.buf[1:2]

    def get(self, what):
        got = self.buf.cpu().tolist()
        assert got[0] == COUNTER_MARGIN and got[2] == COUNTER_MARGIN, what + ": an element next to the counter was written"
        return got[1]


def _xoff(S):
    return 8 if S % 4 == 0 else 3


def _dev(t):
    """a copy on OPS.DEV (a device transfer copies; on the twin the entries would otherwise update the caller's tensor)"""
    return t.clone().to(OPS.DEV)


def _sync():
    if OPS.DEV != "cpu":
        torch.cuda.synchronize()


def _ptr(g):
    from shapegan_amd.lib import ptr
    return None if g is None else ptr(g.view)


# ---- the raw entries, every operand and output guarded ---------------------------------------------------------------------------------------
def raw_forward(x, gamma, beta, rm, rv, v, what, entry="plain", groups=1):
    """sg_bn_train_fwd / sg_bn_eval_fwd (entry "plain"), sg_bn_train_fwd_grouped ("grouped") or sg_bn_train_stats_grouped ("stats").
    Returns the outputs on the CPU and the guarded x (for the backward)."""
    from shapegan_amd.lib import check, stream
    NG, C, S = x.shape
    N = NG // groups
    lib = _lib()
    gx = Guarded(x.shape, x, off=_xoff(S))
    gg, gb = Guarded((C,), gamma), Guarded((C,), beta)
    gy = Guarded(x.shape, off=_xoff(S)) if entry != "stats" else None
    gm, gi = Guarded((groups, C)), Guarded((groups, C))
    running = v["running"]
    grm, grv = (Guarded((C,), rm), Guarded((C,), rv)) if running else (None, None)
    cnt = Counter() if (running and v["training"]) else None
    out = {}
    if v["training"]:
        ws = Workspace(groups * lib.sg_bn_workspace_bytes(C))
        nbt = None if cnt is None else _ptr(cnt)
        if entry == "plain":
            assert groups == 1
            rc = lib.sg_bn_train_fwd(_ptr(gx), _ptr(gg), _ptr(gb), _ptr(gy), _ptr(gm), _ptr(gi), _ptr(grm), _ptr(grv), nbt, N, C, S,
                                     v["eps"], v["momentum"], v["act"], v["slope"], ws.ptr(), ws.nbytes, stream())
        elif entry == "grouped":
            rc = lib.sg_bn_train_fwd_grouped(_ptr(gx), _ptr(gg), _ptr(gb), _ptr(gy), _ptr(gm), _ptr(gi), _ptr(grm), _ptr(grv), nbt, groups,
                                             N, C, S, v["eps"], v["momentum"], v["act"], v["slope"], ws.ptr(), ws.nbytes, stream())
        else:
            gsc, gsh = Guarded((groups, C)), Guarded((groups, C))
            rc = lib.sg_bn_train_stats_grouped(_ptr(gx), _ptr(gg), _ptr(gb), _ptr(gm), _ptr(gi), _ptr(grm), _ptr(grv), nbt, _ptr(gsc),
                                               _ptr(gsh), groups, N, C, S, v["eps"], v["momentum"], ws.ptr(), ws.nbytes, stream())
        check(rc, what)
        _sync()
        ws.check(what)
        if entry == "stats":
            out["scale"], out["shift"] = gsc.get(what + " scale"), gsh.get(what + " shift")
    else:
        check(lib.sg_bn_eval_fwd(_ptr(gx), _ptr(gg), _ptr(gb), _ptr(gy), _ptr(grm), _ptr(grv), _ptr(gm), _ptr(gi), N, C, S, v["eps"],
                                 v["act"], v["slope"], stream()), what)
        _sync()
    if gy is not None:
        out["y"] = gy.get(what + " y")
    out["mean"], out["invstd"] = gm.get(what + " save_mean"), gi.get(what + " save_invstd")
    if running:
        out["rm"], out["rv"] = grm.get(what + " running_mean"), grv.get(what + " running_var")
    if cnt is not None:
        out["nbt"] = cnt.get(what)
    for g in (gx, gg, gb):
        g.intact(what + " (an input)")
    return out, (gx, gg, gb, gm, gi)


def raw_backward(kept, dy, v, what):
    from shapegan_amd.lib import check, stream
    gx, gg, gb, gm, gi = kept
    N, C, S = gx.view.shape
    lib = _lib()
    gdy = Guarded(dy.shape, dy, off=_xoff(S))
    gdx = Guarded(dy.shape, off=_xoff(S))
    gdg, gdb = Guarded((C,)), Guarded((C,))
    ws = Workspace(lib.sg_bn_workspace_bytes(C))
    check(lib.sg_bn_bwd(_ptr(gdy), _ptr(gx), _ptr(gg), _ptr(gb), _ptr(gm), _ptr(gi), _ptr(gdx), _ptr(gdg), _ptr(gdb), N, C, S,
                        1 if v["training"] else 0, v["act"], v["slope"], ws.ptr(), ws.nbytes, stream()), what)
    _sync()
    ws.check(what)
    return {"dx": gdx.get(what + " dx"), "dgamma": gdg.get(what + " dgamma"), "dbeta": gdb.get(what + " dbeta")}


# ---- the same through ops --------------------------------------------------------------------------------------------------------------------
def ops_forward_backward(x, dy, gamma, beta, rm, rv, v):
    from shapegan_amd import ops
    N, C, S = x.shape
    shape = (N, C, S) if S > 1 else (N, C)            # (BatchNorm1d hands over [N, C])
    gx, gdy = Guarded(shape, x, off=_xoff(S)), Guarded(shape, dy, off=_xoff(S))
    xv = gx.view.detach().requires_grad_(True)
    both = v["grads"] == "all"
    g, b = _dev(gamma).requires_grad_(both), _dev(beta).requires_grad_(both)
    running = v["running"]
    r_m, r_v = (_dev(rm), _dev(rv)) if running else (None, None)
    nbt = torch.full((), 3, dtype=torch.long).to(OPS.DEV) if (running and v["training"]) else None
    y = ops.BatchNormAct.apply(xv, g, b, r_m, r_v, nbt, v["training"], v["eps"], v["momentum"], v["act"], v["slope"])
    y.backward(gdy.view)
    _sync()
    out = {"y": y.detach().cpu().reshape(N, C, S), "dx": xv.grad.cpu().reshape(N, C, S)}
    if both:
        out["dgamma"], out["dbeta"] = g.grad.cpu(), b.grad.cpu()
    else:
        assert g.grad is None and b.grad is None
    if running:
        out["rm"], out["rv"] = r_m.cpu(), r_v.cpu()
    if nbt is not None:
        out["nbt"] = int(nbt)
    gx.intact("x of the ops run")
    gdy.intact("dy of the ops run")
    return out


# ---- checks ----------------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b, what):
    assert a.shape == b.shape, what
    assert bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all()), what + ": the two runs differ in bits"


def check_bound(got, want, bound, what, kind):
    """max |got - want| / bound over the elements (0 / 0 = 0): printed, recorded in WORST[kind], asserted <= 1"""
    got, want, bound = got.double(), want.double(), bound.double().expand_as(want)
    assert bool(torch.isfinite(got).all()), what + ": a non-finite value in the output"
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("[bn-forms] %s | %.3g" % (what, worst))
    WORST[kind] = max(WORST.get(kind, 0.0), worst)
    assert worst <= 1.0, "%s: |got - ref| is %.3g of the bound" % (what, worst)


def check_variant(got, ref, v, what, backward=True):
    """got: the outputs of one run (one group's rows of [groups, C] statistics are passed as plain [C] tensors)"""
    hard = "hard" in v
    # (one or two values per channel in training: xhat is 0, or +-1 up to eps, and dx, dgamma, dbeta are the remainders of terms that
    # cancel — dx about 1e-5 of its terms at 2x3x1; the bounds, which know the terms, apply to them, a tolerance relative to the result
    # does not)
    cancelling = v["training"] and ref["y"].shape[0] * ref["y"].shape[2] <= 2
    if "y" in got:
        check_bound(got["y"], ref["y"], ref["fwd_bound"], what + " | y", "fwd")
    if not hard:
        for k in ("y", "mean", "invstd", "scale", "shift"):
            if k in got:
                OPS.close(got[k], ref[k].float(), what=what + " | " + k)
    else:
        for k in ("mean", "invstd", "scale", "shift"):
            if k in got:
                check_bound(got[k], ref[k], ref[k + "_bound"], what + " | " + k, "stats")
    if "rm" in got and "rm" in ref:
        OPS.close(got["rm"], ref["rm"].float(), what=what + " | running_mean")
        OPS.close(got["rv"], ref["rv"].float(), what=what + " | running_var")
    if backward:
        assert ref["dropped"] <= MAX_DROPPED, "%s: %.2f %% of the elements lie in the kink band" % (what, 100 * ref["dropped"])
        WORST["dropped"] = max(WORST.get("dropped", 0.0), ref["dropped"])
        check_bound(got["dx"], ref["dx"], ref["dx_bound"], what + " | dx", "bwd")
        check_bound(got["dgamma"], ref["dgamma"], ref["dgamma_bound"], what + " | dgamma", "bwd")
        check_bound(got["dbeta"], ref["dbeta"], ref["dbeta_bound"], what + " | dbeta", "bwd")
        if not hard and not cancelling:
            for k in ("dx", "dgamma", "dbeta"):
                OPS.close(got[k], ref[k].float(), what=what + " | " + k)


# ---- bodies ----------------------------------------------------------------------------------------------------------------------------------
def body_shape(shape_id):
    """Every variant of one shape: raw (guarded) and through ops, bit for bit the same, against float64."""
    shape = BY_ID[shape_id]
    for v in variants(shape):
        what = "%s | %s" % (shape.id, v["tag"])
        _seed(what + SEEDS.get(what, ""))
        x, dy, gamma, beta, rm, rv = make_inputs(shape, v)
        ref = reference(x, dy, gamma, beta, rm, rv, v)
        dy = ref["dy"]
        raw, kept = raw_forward(x, gamma, beta, rm, rv, v, what)
        raw.update(raw_backward(kept, dy, v, what))
        raw["mean"], raw["invstd"] = raw["mean"][0], raw["invstd"][0]
        via = ops_forward_backward(x, dy, gamma, beta, rm, rv, v)
        for k in via:
            if torch.is_tensor(via[k]):
                same_bits(via[k], raw[k], what + " | " + k + " (ops against the raw entry)")
        if v["training"]:
            if v["running"]:
                assert raw["nbt"] == 4 and via["nbt"] == 4, what + ": num_batches_tracked"
            # the statistics-only entry and the grouped entry with one group: the same bits
            st, _ = raw_forward(x, gamma, beta, rm, rv, v, what + " | stats", entry="stats")
            gr, _ = raw_forward(x, gamma, beta, rm, rv, v, what + " | grouped", entry="grouped")
            for k in ("mean", "invstd", "rm", "rv"):
                if k in raw:
                    same_bits(st[k].reshape(-1), raw[k].reshape(-1), what + " | %s of sg_bn_train_stats_grouped against the fused forward" % k)
                    same_bits(gr[k].reshape(-1), raw[k].reshape(-1), what + " | %s of sg_bn_train_fwd_grouped against the plain entry" % k)
            same_bits(gr["y"], raw["y"], what + " | y of sg_bn_train_fwd_grouped against the plain entry")
            raw["scale"], raw["shift"] = st["scale"][0], st["shift"][0]
        else:
            same_bits(raw["mean"], rm, what + " | save_mean in eval is running_mean")
            assert bool((raw["rm"] == rm).all()) and bool((raw["rv"] == rv).all()), what + ": eval changed the running statistics"
        check_variant(raw, ref, v, what)


def _grouped_reference(shape, groups, x, gamma, beta, rm, rv, v):
    """group after group: the statistics of each, the running statistics carried from one to the next"""
    refs = []
    rm64, rv64 = rm.double(), rv.double()
    for g in range(groups):
        xs = x[g * shape.N:(g + 1) * shape.N]
        r = reference(xs, torch.zeros_like(xs), gamma, beta, rm64, rv64, v)
        rm64, rv64 = r["rm"], r["rv"]
        refs.append(r)
    return refs, rm64, rv64


def body_grouped(gid):
    from shapegan_amd import ops
    groups, per, C, S, nsplit = GROUPED_BY_ID[gid]
    assert ops.bn_plan(per, C, S)[0] == nsplit
    shape = Shape(per, C, S, (nsplit, 0), (0, 0), "one group")
    for act, slope in TWO_ACTS:
        v = dict(training=True, act=act, slope=slope, momentum=0.1, eps=1e-5, running=True, tag="grouped-" + ACT_NAMES[act])
        what = "%s | %s" % (gid, v["tag"])
        _seed(what)
        x, _, gamma, beta, rm, rv = make_inputs(shape, v, groups)
        refs, rm_ref, rv_ref = _grouped_reference(shape, groups, x, gamma, beta, rm, rv, v)
        fw, _ = raw_forward(x, gamma, beta, rm, rv, v, what + " | fwd", entry="grouped", groups=groups)
        st, _ = raw_forward(x, gamma, beta, rm, rv, v, what + " | stats", entry="stats", groups=groups)
        # through ops (the same bits)
        dev = _dev
        for entry in ("fwd", "stats"):
            r_m, r_v, nbt = dev(rm), dev(rv), torch.full((), 3, dtype=torch.long).to(OPS.DEV)
            gx = Guarded(x.shape, x, off=_xoff(S))
            if entry == "fwd":
                y = ops.bn_train_fwd_grouped_raw(gx.view, dev(gamma), dev(beta), r_m, r_v, nbt, v["eps"], v["momentum"], act, slope, groups)
                same_bits(y.cpu(), fw["y"], what + " | y (ops against the raw entry)")
            else:
                sc, sh = ops.bn_train_stats_affine(gx.view, dev(gamma), dev(beta), r_m, r_v, nbt, v["eps"], v["momentum"], groups)
                same_bits(sc.cpu().reshape(groups, C), st["scale"], what + " | scale (ops against the raw entry)")
                same_bits(sh.cpu().reshape(groups, C), st["shift"], what + " | shift (ops against the raw entry)")
            same_bits(r_m.cpu(), fw["rm"], what + " | running_mean (ops against the raw entry)")
            same_bits(r_v.cpu(), fw["rv"], what + " | running_var (ops against the raw entry)")
            assert int(nbt) == 3 + groups
        for k in ("mean", "invstd", "rm", "rv"):
            same_bits(st[k], fw[k], what + " | %s of the statistics entry against the fused forward" % k)
        assert fw["nbt"] == 3 + groups and st["nbt"] == 3 + groups, what + ": num_batches_tracked"
        for g in range(groups):
            got = {"y": fw["y"][g * per:(g + 1) * per], "mean": fw["mean"][g], "invstd": fw["invstd"][g], "scale": st["scale"][g],
                   "shift": st["shift"][g]}
            check_variant(got, refs[g], v, "%s | group %d" % (what, g), backward=False)
        OPS.close(fw["rm"], rm_ref.float(), what=what + " | running_mean")
        OPS.close(fw["rv"], rv_ref.float(), what=what + " | running_var")


def _refused(call, outputs, rc_want, message, what):
    rc = call()
    _sync()
    assert rc == rc_want, "%s: returned %d, not %d" % (what, rc, rc_want)
    for g in outputs:
        g.untouched(what)
    from shapegan_amd import lib as L
    last = L._load_hip().sg_last_error() if OPS.DEV != "cpu" else L.load_cpu().sg_cpu_last_error()
    assert message in last, (what, last)


def body_refusals():
    """groups = 65 and S = 0 are refused as arguments, a workspace one byte short as a workspace (the twin takes none); no output is
    touched."""
    from shapegan_amd.lib import stream
    lib = _lib()
    N, C, S = 2, 3, 8
    _seed("refusals")
    for groups, short, S_ in ((65, 0, S), (2, 1, S), (64, 1, S), (2, 0, 0)):
        if short and OPS.DEV == "cpu":
            continue
        Sx = max(S_, 1)
        x = torch.randn(groups * N, C, Sx)
        gx, gg, gb = Guarded(x.shape, x, off=8), Guarded((C,), torch.ones(C)), Guarded((C,), torch.zeros(C))
        grm, grv = Guarded((C,), torch.zeros(C)), Guarded((C,), torch.ones(C))
        nbytes = groups * lib.sg_bn_workspace_bytes(C) - short
        want = (SG_ERR_WORKSPACE, b"workspace too small") if short else (SG_ERR_ARG, b"")
        for entry in ("fwd", "stats", "plain", "eval", "bwd"):
            if entry in ("plain", "eval", "bwd") and (groups != 2 or (entry == "eval" and short)):
                continue
            outs = [Guarded(x.shape, off=8)] + [Guarded((groups, C)) for _ in range(4)] + [Guarded((C,)), Guarded((C,))]
            gy, gm, gi, gsc, gsh, gdg, gdb = outs
            ws = Workspace(nbytes)
            cnt = Counter()
            what = "refusal %s groups %d short %d S %d" % (entry, groups, short, S_)
            if entry == "fwd":
                call = lambda: lib.sg_bn_train_fwd_grouped(_ptr(gx), _ptr(gg), _ptr(gb), _ptr(gy), _ptr(gm), _ptr(gi), _ptr(grm), _ptr(grv),  # noqa: E731
                                                           _ptr(cnt), groups, N, C, S_, 1e-5, 0.1, LEAKY, 0.2, ws.ptr(), ws.nbytes, stream())
            elif entry == "stats":
                call = lambda: lib.sg_bn_train_stats_grouped(_ptr(gx), _ptr(gg), _ptr(gb), _ptr(gm), _ptr(gi), _ptr(grm), _ptr(grv), _ptr(cnt),  # noqa: E731
                                                             _ptr(gsc), _ptr(gsh), groups, N, C, S_, 1e-5, 0.1, ws.ptr(), ws.nbytes, stream())
            elif entry == "plain":      # (one group of 2 N samples; the workspace of one group, one byte short)
                ws = Workspace(lib.sg_bn_workspace_bytes(C) - short)
                call = lambda: lib.sg_bn_train_fwd(_ptr(gx), _ptr(gg), _ptr(gb), _ptr(gy), _ptr(gm), _ptr(gi), _ptr(grm), _ptr(grv), _ptr(cnt),  # noqa: E731
                                                   2 * N, C, S_, 1e-5, 0.1, LEAKY, 0.2, ws.ptr(), ws.nbytes, stream())
            elif entry == "eval":
                call = lambda: lib.sg_bn_eval_fwd(_ptr(gx), _ptr(gg), _ptr(gb), _ptr(gy), _ptr(grm), _ptr(grv), _ptr(gm), _ptr(gi), 2 * N, C, S_,  # noqa: E731
                                                  1e-5, LEAKY, 0.2, stream())
            else:
                ws = Workspace(lib.sg_bn_workspace_bytes(C) - short)
                call = lambda: lib.sg_bn_bwd(_ptr(gx), _ptr(gx), _ptr(gg), _ptr(gb), _ptr(grm), _ptr(grv), _ptr(gy), _ptr(gdg), _ptr(gdb),  # noqa: E731
                                             2 * N, C, S_, 1, LEAKY, 0.2, ws.ptr(), ws.nbytes, stream())
            _refused(call, outs, want[0], want[1], what)
            ws.check(what)
            assert cnt.get(what) == 3, what + ": the counter moved"
            assert bool((grm.view == 0).all()) and bool((grv.view == 1).all()), what + ": the running statistics moved"


# ---- calibration (not a test: run by hand on the CPU) -----------------------------------------------------------------------------------------
def torch_fp32_ratios():
    """The largest ratio of torch's own fp32 F.batch_norm + autograd (CPU) against the bounds above with K = 1, over the table."""
    worst = {"fwd": 0.0, "bwd": 0.0}
    for shape in SHAPES:
        for v in variants(shape):
            if shape.N * shape.S == 1 and v["training"]:
                continue          # torch raises
            what = "%s | %s" % (shape.id, v["tag"])
            _seed(what + SEEDS.get(what, ""))
            x, dy, gamma, beta, rm, rv = make_inputs(shape, v)
            ref = reference(x, dy, gamma, beta, rm, rv, v)
            xt, g, b = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
            z = F.batch_norm(xt, rm.clone(), rv.clone(), g, b, v["training"], v["momentum"], v["eps"])
            y = _act64(z, v["act"], v["slope"])
            y.backward(ref["dy"])
            r = {"fwd": ((y.detach().double() - ref["y"]).abs() / (ref["fwd_bound"] / K_FWD)).max()}
            r["bwd"] = 0.0
            for k, t in (("dx", xt.grad), ("dgamma", g.grad), ("dbeta", b.grad)):
                err = (t.double() - ref[k]).abs()
                bound = (ref[k + "_bound"] / K_BWD).expand_as(err)
                r["bwd"] = max(r["bwd"], float(torch.where(err == 0, torch.zeros_like(err), err / bound).max()))
            print("[bn-forms] torch fp32 | %s | fwd %.3g | bwd %.3g | dropped %.4f" % (what, float(r["fwd"]), r["bwd"], ref["dropped"]))
            worst = {k: max(worst[k], float(r[k])) for k in worst}
    return worst
