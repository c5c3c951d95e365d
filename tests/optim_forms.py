"""Case tables, float64 references, bounds and test bodies for the fused optimizers and the elementwise kernels (K5, K8 - K11,
shapegan_amd/csrc/elementwise.hip) in every calling form (tests/test_gpu_optim_forms.py; the bodies are re-run on the twin by
tests/test_cpu_twin.py; the float64 formulas are held against torch.optim in float64 by tests/test_optim_forms_host.py).  Pure
Python: nothing here is a test by itself.

Forms.  Every kernel runs (1) through its Python caller (optim.RMSprop, optim.Adam, optim.step_together, ops.Act, ops.gather_rows,
ops.mean, Discriminator.clip_weights; sg_axpby and sg_clamp have no caller of their own and run raw only) and (2) "raw", through the
library entry with every operand and output inside a larger buffer whose margins hold NaN (-7 around the Adam counter, the ticket
words and the guard word; the reduce workspace of exactly the byte count asked for between two fences, gemm_forms.Workspace).  The
margins must be unchanged afterwards and the two runs agree bit for bit (scatter_add_rows, whose atomics arrive in any order, is
held to its bound in both).  Operands are 16-byte aligned, as every caller provides; sg_reduce_sum tests its own alignment and runs
at element offsets 0, 1, 2, 3.

Reference.  The float64 formula written out in torch from the SAME fp32 inputs and the fp32-rounded hyperparameters.  In a case of
several steps the reference restarts from the kernel's own state before each step: errors do not compound, one wrong step shows.

Bounds, element-wise, u = 2^-24, from float64 reference quantities only (s = grad_scale, c = 1 - beta, primes = after the step):
  Adam      |m' - ref| <= K u (|b1 m| + |c1 g s|)         |v' - ref| <= K u (b2 v + c2 (g s)^2)
            |p' - ref| <= K u (|p| + (lr / bc1) (|b1 m| + |c1 g s|) / denom_ref)    (the last term carries the cancellation in m')
  RMSprop   |sq' - ref| <= K u (alpha sq + (1 - alpha) (g s)^2)       |p' - ref| <= K u (|p| + lr |g s| / (sqrt(sq') + eps))
            with the clip on, against the clamped reference (a clamp does not enlarge a distance), and EQUAL to +-clip wherever
            the unclamped float64 value lies beyond +-clip by more than the bound
  corr[0], corr[1] of the device counter: within 1 ulp of float(1 - b1^t), float(sqrt(1 - b2^t)) from float64 pow (the kernel's
            repeated squaring is a few ulp of double before rounding); m', v' of the device-counter entry are the host-counter
            entry's bit for bit, p' within one ulp of the bound's terms, 2 u (|p| + ...)  (ulp of 1.0 = 2 u)
  sg_reduce_sum      u |ref| + n 2^-53 sum|x| |scale|          (a float accumulation of the cancelling data fails it)
  scatter_add_rows   (count_r - 1) u sum|terms of row r|       sg_axpby   2 u (|a x| + |b y|)
  gather_rows, sg_clamp, sg_clamp_multi: bit-equal to torch;  dx of act_bwd_rowsum: bit-equal to act_bwd on the same inputs
  activations   forward K_ACT u |ref| + FLT_MIN; backward from the fp32 y the kernel is given K_ACT u |dy| (1 + y^2) for tanh,
            K_ACT u |dy| (|y| + y^2) for sigmoid, 2 u |dy| otherwise; row sums K_ACT u sum|dx| over the row.  The backward bound
            carries an absolute floor of 2^-148 that the issue's formula lacks: for x in [-88.7, -87.3] the kernels' own sigmoid
            is a denormal y, dy y (1 - y) is rounded twice onto the denormal grid (half a step of 2^-149 each) and no fp32 code,
            torch's included, can be u-relative there (first seen at act-2097155 on the twin: 41 of the bound without the floor).

K and K_ACT are not fitted to the kernels.  torch's own fp32 CPU optimizers (torch.optim.Adam / RMSprop given the fp32-rounded
hyperparameters, stepped from their own states over this file's final case table, torch_fp32_ratios() below) reach 3.77 of the K = 1
bound (Adam p; m 2.16, v 2.63; RMSprop p 3.75, sq 2.83), torch's fp32 activations and their autograd 2.43 (sigmoid forward; backward
2.38, row sums 1.43).  4 x that, for a different and equally valid rounding order, rounded up to a power of two: K = 16, K_ACT = 16.
Every check prints `[optim-forms] case | output | max ratio` before it asserts.  Largest ratios of the kernels over the table:
                 adam.m   adam.v   adam.p   rms.sq   rms.p    act.fwd  act.bwd  act.rowsum  reduce   scatter  axpby
    twin         0.145    0.17     0.165    0.188    0.205    0.249    0.229    0.123       0.665    0.295    0.937
    MI355X       0.127    0.169    0.189    0.205    0.23     0.249    0.229    0.123       0.665      0.285    0.937
(sg_axpby's and sg_reduce_sum's bounds are derived, not scaled by K: a result's own rounding alone may use half of them.)  The p of
the device-counter entry was the host-counter entry's bit for bit in every case, on both.

Element kinds of the optimizer cases, interleaved (element i has kind i mod 9, so every kind falls in every workgroup): 0 N(0,1)
gradients; 1 g = 0 with zero state (p must keep its bits); 2 g = 0 with non-zero moments; 3 |g| = 1e-10 and 4 |g| = 1e-8 from zero
state (eps dominates / ties); 5 |g| = 1e15; 6 b1 m ~ -c1 g s (to 1e-6; N(0,1) where there is no first moment); 7 |p| = 1e4 with an
update below its ulp; 8 v >> g^2.  With the clip on, p is drawn at the scale of the clip so that elements end on both sides of it.

The finding.  clamp_kernel, clamp_multi_kernel and the clip of rmsprop_kernel were fminf(fmaxf(v, lo), hi), and fmaxf(NaN, lo) is lo:
a NaN critic weight became -clip and stayed there (square_avg stays NaN), where the reference's p.data.clamp_ and the twin keep the
NaN.  That is read from the parent's code (its library was not run): there the cases clamp-1, clamp-513, clamp-1048577, every
clamp_multi case, body_clip_nan and nonfinite-rmsprop-clip0.01 feed a NaN through those expressions, on the GPU alone.  The kernels
now clamp as voxel_prepare_kernel does (one shared helper); finite values keep the parent's bits (bit-equality with torch.clamp).  The twin's sg_adam_step_dev_multi updated the
sets in front of a null entry before refusing it (multi refusals); it now looks at every set first, as the library does.

The twin's Adam is not lane-faithful: it has no tickets, derives the corrections with pow, and leaves the contraction of
b2 v + c2 g g to the compiler.  It is held to the same bounds, not to the kernels' bits.
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import test_gpu_ops as OPS
from batchnorm_forms import Guarded, same_bits, _dev, _seed, _sync
from gemm_forms import Workspace

U = 2.0 ** -24
K = 16.0
K_ACT = 16.0
FLT_MIN = 2.0 ** -126
DENORM_FLOOR = 2.0 ** -148          # two roundings onto the denormal grid, half a step of 2^-149 each
SENTINEL = -7
SG_ERR_ARG = -1
NONE, LEAKY, RELU, TANH, SIGMOID = 0, 1, 2, 3, 4
ADAM_DEV_WORDS = 544
WORST = {}          # output -> the largest ratio seen in this process


def _lib():
    from shapegan_amd import ops
    return ops._lib()


def P(g):
    from shapegan_amd.lib import ptr
    return None if g is None else ptr(g.view)


def f32(x):
    """the value a float argument has after the call has rounded it to fp32"""
    return float(torch.tensor(x, dtype=torch.float32))


class Words(object):
    """`n` integers inside a larger buffer whose margins hold SENTINEL (8 words in front: 32 or 64 bytes)"""

    def __init__(self, n, dtype, values=0, off=8, tail=8):
        buf = torch.full((off + n + tail,), SENTINEL, dtype=dtype)
        buf[off:off + n] = values
        self.off, self.n = off, n
        self.buf = buf.clone().to(OPS.DEV)
        self.view = self.buf[off:off + n]

    def get(self, what):
        got = self.buf.cpu()
        ok = bool((got[:self.off] == SENTINEL).all()) and bool((got[self.off + self.n:] == SENTINEL).all())
        assert ok, what + ": a word outside the window was written"
        return got[self.off:self.off + self.n].clone()


def G32(values, off=8):
    """a flat fp32 operand inside a NaN buffer, 16-byte aligned"""
    return Guarded((values.numel(),), values, off=off)


def check_bound(got, want, bound, what, key, mask=None):
    """max |got - want| / bound over the elements (0 / 0 = 0): printed, recorded in WORST[key], asserted <= 1"""
    want = want.double()
    got, bound = got.double().reshape(want.shape).reshape(-1), bound.double().expand_as(want).reshape(-1)
    want = want.reshape(-1)
    if mask is not None:
        got, want, bound = got[mask], want[mask], bound[mask]
    assert bool(torch.isfinite(got).all()), "%s | %s: a non-finite value in the output" % (what, key)
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("[optim-forms] %s | %s | %.3g" % (what, key, worst))
    WORST[key] = max(WORST.get(key, 0.0), worst)
    assert worst <= 1.0, "%s | %s: |got - ref| is %.3g of the bound" % (what, key, worst)


def same_pattern(got, want, what):
    """the finiteness pattern: NaN, +inf, -inf or finite, element by element"""
    for name, fn in (("NaN", torch.isnan), ("+inf", torch.isposinf), ("-inf", torch.isneginf)):
        assert bool((fn(got) == fn(want)).all()), "%s: %s where torch fp32 has none, or the reverse (%s against %s)" % (
            what, name, got.tolist(), want.tolist())


# ---- optimizer cases ----------------------------------------------------------------------------------------------------------------------
NK = 9
SMALL_N = [1, 3, 257, 513, 7680, 7681, 8193, 16384, 16385]          # workgroups: 1, 1, 1, 2, 15, 16, 17, 32, 33
LARGE_N = [1048576, 1048577, 2621447]                                # 2048 workgroups: one round exactly, a second, a partial third
ALL_N = SMALL_N + LARGE_N
TWIN_N = SMALL_N + [1048577]
EPS = 1e-8
ADAM_HYPER = [(1e-3, 0.9, 0.999), (5e-3, 0.8, 0.99), (2e-4, 0.5, 0.999), (1e-3, 0.0, 0.999)]
SCALES = [1.0, 0.125, 1.0 / 3.0]
FIRST_STEPS = [1, 2, 1000, 37]
RMS_HYPER = [(lr, alpha, clip) for (lr, alpha) in ((1e-3, 0.99), (5e-5, 0.9)) for clip in (0.0, 0.01, 0.5)]
COUNTER_PRESETS = [0, 1, 9, 999, 65535, 10 ** 6, 2 ** 31 + 5]


def workgroups(n):
    return min((n + 511) // 512, 2048)


def adam_cases(n):
    """(hyper index, grad_scale, first step, steps): every hyperparameter set at the small sizes with five steps, one set and two
    steps at the large ones (a step there costs a float64 reference over millions of elements); scales and first steps rotate"""
    i = ALL_N.index(n)
    if n in SMALL_N:
        return [(h, SCALES[(h + i) % 3], FIRST_STEPS[(h + i) % 4], 5) for h in range(4)]
    return [(i % 4, SCALES[i % 3], FIRST_STEPS[i % 4], 2)]


def rms_cases(n):
    i = ALL_N.index(n)
    if n in SMALL_N:
        return [(r, SCALES[(r + i) % 3], 5) for r in range(6)]
    return [((2 * i + 1) % 6, SCALES[i % 3], 2)]


def _kinds(n):
    return torch.arange(n) % NK


def _signs(n):
    return torch.where(torch.rand(n) < 0.5, -torch.ones(n), torch.ones(n))


def make_state(n, clip=0.0):
    """fp32 p, m, v (v is RMSprop's square_avg) by element kind"""
    k = _kinds(n)
    p = torch.randn(n) * (clip if clip > 0 else 1.0)
    m = torch.randn(n) * 0.1
    v = torch.rand(n) * 0.01 + 1e-4
    zero = (k == 1) | (k == 3) | (k == 4)
    m[zero], v[zero] = 0.0, 0.0
    p[k == 7] = (_signs(n) * 1e4)[k == 7]
    m[k == 7], v[k == 7] = 0.0, 1.0
    v[k == 8] = 1e6
    return p, m, v


def make_grad(n, m, b1, s):
    """fp32 g by element kind; m: the first moment the step will start from (None: RMSprop)"""
    k = _kinds(n)
    g = torch.randn(n)
    sg = _signs(n)
    g[(k == 1) | (k == 2)] = 0.0
    for kind, mag in ((3, 1e-10), (4, 1e-8), (5, 1e15)):
        g[k == kind] = (sg * mag)[k == kind]
    if m is not None and b1 > 0:
        sel = k == 6
        g[sel] = (-(b1 * m[sel].double()) / ((1 - b1) * s) * (1 + 1e-6 * torch.randn(int(sel.sum())).double())).float()
    g[k == 7] *= 0.1
    return g


# ---- float64 formulas -----------------------------------------------------------------------------------------------------------------------
def adam_formula(p, g, m, v, lr, b1, b2, eps, t, s=1.0):
    """One step of torch.optim.Adam (defaults) in float64; also the magnitudes of the bounds."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gs = g * s
    c1, c2 = 1.0 - b1, 1.0 - b2
    m1 = b1 * m + c1 * gs
    v1 = b2 * v + c2 * gs * gs
    bc1, bc2_sqrt = 1.0 - b1 ** t, (1.0 - b2 ** t) ** 0.5
    denom = v1.sqrt() / bc2_sqrt + eps
    p1 = p - (lr / bc1) * m1 / denom
    mmag = (b1 * m).abs() + (c1 * gs).abs()
    return {"p": p1, "m": m1, "v": v1, "m_mag": mmag, "v_mag": v1, "p_mag": p.abs() + (lr / bc1) * mmag / denom,
            "bc1": bc1, "bc2_sqrt": bc2_sqrt}


def rms_formula(p, g, sq, lr, alpha, eps, s=1.0, clip=0.0):
    """One step of torch.optim.RMSprop (defaults) in float64, then the clamp to +-clip (clip > 0); also the bounds' magnitudes."""
    p, g, sq = p.double(), g.double(), sq.double()
    gs = g * s
    sq1 = alpha * sq + (1.0 - alpha) * gs * gs
    denom = sq1.sqrt() + eps
    raw = p - lr * gs / denom
    return {"p": raw.clamp(-clip, clip) if clip > 0 else raw, "raw": raw, "sq": sq1, "sq_mag": sq1, "p_mag": p.abs() + lr * gs.abs() / denom}


def _h32(h):
    return tuple(f32(x) for x in h)


def check_adam_step(got, prev, g, h, t, s, what, skip=None):
    """got / prev: (p, m, v) fp32 on the CPU after / before the step; skip: elements left out of the bounds (non-finite cases)"""
    lr, b1, b2 = _h32(h)
    ref = adam_formula(prev[0], g, prev[1], prev[2], lr, b1, b2, f32(EPS), t, f32(s))
    mask = None if skip is None else ~skip
    check_bound(got[1], ref["m"], K * U * ref["m_mag"], what, "adam.m", mask)
    check_bound(got[2], ref["v"], K * U * ref["v_mag"], what, "adam.v", mask)
    check_bound(got[0], ref["p"], K * U * ref["p_mag"], what, "adam.p", mask)
    still = _kinds(g.numel()) == 1
    if skip is not None:
        still = still & ~skip
    same_bits(got[0][still], prev[0][still], what + " | p of the elements with g = 0 and zero state")
    return ref


def check_rms_step(got, prev, g, r, s, what, skip=None):
    lr, alpha, clip = _h32(r)
    ref = rms_formula(prev[0], g, prev[1], lr, alpha, f32(EPS), f32(s), clip)
    mask = None if skip is None else ~skip
    check_bound(got[1], ref["sq"], K * U * ref["sq_mag"], what, "rms.sq", mask)
    bound = K * U * ref["p_mag"]
    check_bound(got[0], ref["p"], bound, what, "rms.p", mask)
    still = _kinds(g.numel()) == 1
    if clip > 0:
        beyond = ((ref["raw"] - clip).abs() > bound) & ((ref["raw"] + clip).abs() > bound) & (ref["raw"].abs() > clip)
        if skip is not None:
            beyond = beyond & ~skip
        want = torch.where(ref["raw"] > 0, torch.full_like(ref["raw"], clip), torch.full_like(ref["raw"], -clip)).float()
        same_bits(got[0][beyond], want[beyond], what + " | p beyond the clip by more than the bound")
        still = still & (prev[0].abs() <= clip)
    if skip is not None:
        still = still & ~skip
    same_bits(got[0][still], prev[0][still], what + " | p of the elements with g = 0 and zero state")
    return ref


# ---- steppers: the kernels raw, and torch's fp32 optimizers (calibration) ---------------------------------------------------------------------
class RawAdam(object):
    """sg_adam_step[_guarded] (dev False) or sg_adam_step_dev[_guarded] (dev True) on guarded buffers"""

    def __init__(self, p, m, v, h, s, dev=False, counter=0, guard=None):
        self.n, self.h, self.s, self.dev, self.guard = p.numel(), h, s, dev, guard
        self.P, self.M, self.V = G32(p), G32(m), G32(v)
        self.G = G32(torch.zeros_like(p))
        if dev:
            self.cnt = Words(1, torch.int64, counter)
            self.corr = Words(ADAM_DEV_WORDS, torch.int32, 0)

    def step(self, g, t, what):
        from shapegan_amd.lib import check, stream
        lib = _lib()
        self.G.view.copy_(g)
        lr, b1, b2 = self.h
        a = (P(self.P), P(self.G), P(self.M), P(self.V), self.n, lr, b1, b2, EPS)
        if self.dev:
            if self.guard is None:
                rc = lib.sg_adam_step_dev(*a, P(self.cnt), P(self.corr), self.s, stream())
            else:
                rc = lib.sg_adam_step_dev_guarded(*a, P(self.cnt), P(self.corr), self.s, P(self.guard), stream())
        elif self.guard is None:
            rc = lib.sg_adam_step(*a, t, self.s, stream())
        else:
            rc = lib.sg_adam_step_guarded(*a, t, self.s, P(self.guard), stream())
        check(rc, what)
        _sync()
        self.G.intact(what + " g")
        return self.state(what)

    def state(self, what):
        return self.P.get(what + " p"), self.M.get(what + " m"), self.V.get(what + " v")

    def words(self, what):
        """(counter, corr[0], corr[1], the ticket words)"""
        w = self.corr.get(what + " corr")
        return int(self.cnt.get(what + " counter")[0]), float(w[:2].view(torch.float32)[0]), float(w[:2].view(torch.float32)[1]), w[2:]


class RawRms(object):
    def __init__(self, p, sq, r, s):
        self.n, self.r, self.s = p.numel(), r, s
        self.P, self.S, self.G = G32(p), G32(sq), G32(torch.zeros_like(p))

    def step(self, g, what):
        from shapegan_amd.lib import check, stream
        self.G.view.copy_(g)
        lr, alpha, clip = self.r
        check(_lib().sg_rmsprop_step(P(self.P), P(self.G), P(self.S), self.n, lr, alpha, EPS, self.s, clip, stream()), what)
        _sync()
        self.G.intact(what + " g")
        return self.P.get(what + " p"), self.S.get(what + " square_avg")


def torch_adam_step(p, g, m, v, h, t, s):
    """(torch keeps its hyperparameters in double: it is given the fp32-rounded ones, which the kernels and the reference use)"""
    par = torch.nn.Parameter(p.clone())
    h = _h32(h)
    opt = torch.optim.Adam([par], lr=h[0], betas=(h[1], h[2]), eps=f32(EPS), foreach=False)
    opt.state[par] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    par.grad = g * torch.tensor(s, dtype=torch.float32)
    opt.step()
    return par.data.clone(), opt.state[par]["exp_avg"].clone(), opt.state[par]["exp_avg_sq"].clone()


def torch_rms_step(p, g, sq, r, s):
    par = torch.nn.Parameter(p.clone())
    r = _h32(r)
    opt = torch.optim.RMSprop([par], lr=r[0], alpha=r[1], eps=f32(EPS), foreach=False)
    opt.state[par] = {"step": torch.tensor(0.0), "square_avg": sq.clone()}
    par.grad = g * torch.tensor(s, dtype=torch.float32)
    opt.step()
    if r[2] > 0:
        par.data.clamp_(-r[2], r[2])
    return par.data.clone(), opt.state[par]["square_avg"].clone()


# ---- the Python callers -------------------------------------------------------------------------------------------------------------------------
def adam_via_optim(p, m, v, grads, h, t0, s, capturable):
    """optim.Adam over one parameter of n elements from the given state (its flat buffers round n up to a multiple of 4)"""
    from shapegan_amd import optim
    n = p.numel()
    par = torch.nn.Parameter(_dev(p))
    opt = optim.Adam([par], lr=h[0], betas=(h[1], h[2]), eps=EPS, capturable=capturable)
    opt.exp_avg[:n].copy_(m)
    opt.exp_avg_sq[:n].copy_(v)
    opt.grad_scale = s
    if capturable:
        opt.step_dev.fill_(t0 - 1)
    else:
        opt.steps = [t0 - 1]
    for g in grads:
        par.grad.copy_(g)
        opt.step()
    _sync()
    return opt, (par.data.detach().cpu().clone(), opt.exp_avg[:n].cpu().clone(), opt.exp_avg_sq[:n].cpu().clone())


def rms_via_optim(p, sq, grads, r, s):
    from shapegan_amd import optim
    n = p.numel()
    par = torch.nn.Parameter(_dev(p))
    opt = optim.RMSprop([par], lr=r[0], alpha=r[1], eps=EPS, clip=r[2])
    opt.square_avg[:n].copy_(sq)
    opt.grad_scale = s
    for g in grads:
        par.grad.copy_(g)
        opt.step()
    _sync()
    return par.data.detach().cpu().clone(), opt.square_avg[:n].cpu().clone()


def ulp_apart(got, want64):
    """|got - float(want64)| in ulps of float(want64)"""
    want = np.float32(want64)
    return abs(float(np.float32(got)) - float(want)) / float(np.spacing(want))


def check_dev_words(run, t, h, what):
    cnt, c0, c1, tickets = run.words(what)
    _, b1, b2 = _h32(h)
    assert cnt == t, "%s: the counter is %d, not %d" % (what, cnt, t)
    a0, a1 = ulp_apart(c0, 1.0 - b1 ** t), ulp_apart(c1, (1.0 - b2 ** t) ** 0.5)
    print("[optim-forms] %s | corr ulps | %g %g" % (what, a0, a1))
    assert a0 <= 1 and a1 <= 1, "%s: corr = (%r, %r) is (%g, %g) ulp from float64 pow" % (what, c0, c1, a0, a1)
    assert bool((tickets == 0).all()), what + ": a ticket word was left non-zero"


def check_dev_against_host(dev, host, ref, what):
    """the first step from one state: m', v' the same bits, p' within one ulp (2 u) of the bound's terms"""
    same_bits(dev[1], host[1], what + " | m of the device-counter entry against the host-counter entry")
    same_bits(dev[2], host[2], what + " | v of the device-counter entry against the host-counter entry")
    check_bound(dev[0], host[0].double(), 2 * U * ref["p_mag"], what, "adam.p dev against host")


# ---- bodies: optimizers ---------------------------------------------------------------------------------------------------------------------------
def body_adam(n):
    """Every case of one length: the host-counter and the device-counter entry, raw with bounds after every step, and through
    optim.Adam (capturable or not) bit for bit."""
    for hi, s, t0, steps in adam_cases(n):
        h = ADAM_HYPER[hi]
        what = "adam n=%d (%d wg) h%d s%.3g t0=%d" % (n, workgroups(n), hi, s, t0)
        _seed(what)
        p0, m0, v0 = make_state(n)
        host = RawAdam(p0, m0, v0, h, s)
        dev = RawAdam(p0, m0, v0, h, s, dev=True, counter=t0 - 1)
        sh, sd, grads = (p0, m0, v0), (p0, m0, v0), []
        for k in range(steps):
            t = t0 + k
            g = make_grad(n, sh[1], f32(h[1]), f32(s))
            grads.append(g)
            w = "%s | step %d" % (what, k)
            nh = host.step(g, t, w + " | host")
            ref = check_adam_step(nh, sh, g, h, t, s, w + " | host")
            nd = dev.step(g, t, w + " | dev")
            check_dev_words(dev, t, h, w + " | dev")
            if k == 0:
                check_dev_against_host(nd, nh, ref, w)
            else:
                same_bits(nd[1], nh[1], w + " | m (dev against host)")      # m and v never see the corrections
                same_bits(nd[2], nh[2], w + " | v (dev against host)")
                check_adam_step(nd, sd, g, h, t, s, w + " | dev")
            sh, sd = nh, nd
        for capturable, raw in ((False, sh), (True, sd)):
            opt, via = adam_via_optim(p0, m0, v0, grads, h, t0, s, capturable)
            for name, a, b in zip("pmv", via, raw):
                same_bits(a, b, "%s | %s (optim.Adam capturable=%s against the raw entry)" % (what, name, capturable))
            if capturable:
                assert int(opt.step_dev.cpu()[0]) == t0 + steps - 1, what + ": optim.Adam's device counter"
                assert bool((opt.corr_dev.cpu().view(torch.int32)[2:] == 0).all()), what + ": optim.Adam's ticket words"


def body_rmsprop(n):
    for ri, s, steps in rms_cases(n):
        r = RMS_HYPER[ri]
        what = "rmsprop n=%d (%d wg) lr=%g alpha=%g clip=%g s%.3g" % (n, workgroups(n), r[0], r[1], r[2], s)
        _seed(what)
        p0, _, sq0 = make_state(n, r[2])
        run = RawRms(p0, sq0, r, s)
        st, grads = (p0, sq0), []
        for k in range(steps):
            g = make_grad(n, None, 0.0, f32(s))
            grads.append(g)
            new = run.step(g, "%s | step %d" % (what, k))
            check_rms_step(new, st, g, r, s, "%s | step %d" % (what, k))
            st = new
        via = rms_via_optim(p0, sq0, grads, r, s)
        same_bits(via[0], st[0], what + " | p (optim.RMSprop against the raw entry)")
        same_bits(via[1], st[1], what + " | square_avg (optim.RMSprop against the raw entry)")


NONFINITE = ["adam", "adam-dev", "rmsprop-clip0", "rmsprop-clip0.01"]
NONFINITE_AT = [5, 4000, 8192]              # NaN, +inf, 1e20 (its square overflows fp32): first, middle and last workgroup


def body_nonfinite(kind):
    """n = 8193 with a NaN, a +inf and a 1e20 gradient on zero state at step 1: every other element meets its bound, the three have
    the finiteness pattern of torch's fp32 optimizer (RMSprop followed by p.data.clamp_, as the reference trains)."""
    n, s = 8193, 1.0
    what = "nonfinite-" + kind
    _seed(what)
    bad = torch.tensor([float("nan"), float("inf"), 1e20])
    at = torch.tensor(NONFINITE_AT)
    skip = torch.zeros(n, dtype=torch.bool)
    skip[at] = True
    if kind.startswith("adam"):
        h = ADAM_HYPER[0]
        p0, m0, v0 = make_state(n)
        m0[at], v0[at] = 0.0, 0.0
        g = make_grad(n, m0, f32(h[1]), s)
        g[at] = bad
        run = RawAdam(p0, m0, v0, h, s, dev=kind == "adam-dev")
        got = run.step(g, 1, what)
        check_adam_step(got, (p0, m0, v0), g, h, 1, s, what, skip)
        want = torch_adam_step(p0[at], g[at], m0[at], v0[at], h, 1, s)
        _, via = adam_via_optim(p0, m0, v0, [g], h, 1, s, kind == "adam-dev")
        names = "pmv"
    else:
        r = (1e-3, 0.99, float(kind.split("clip")[1]))
        p0, _, v0 = make_state(n, r[2])
        v0[at] = 0.0
        g = make_grad(n, None, 0.0, s)
        g[at] = bad
        got = RawRms(p0, v0, r, s).step(g, what)
        check_rms_step(got, (p0, v0), g, r, s, what, skip)
        want = torch_rms_step(p0[at], g[at], v0[at], r, s)
        via = rms_via_optim(p0, v0, [g], r, s)
        names = ["p", "square_avg"]
    for name, a, b, c in zip(names, got, want, via):
        same_pattern(a[at], b, "%s | %s at the NaN, +inf and 1e20 gradients" % (what, name))
        same_bits(c, a, "%s | %s (the Python caller against the raw entry)" % (what, name))


def body_dev_counter(preset):
    """One step of sg_adam_step_dev at n = 8193 from a preset counter: the counter, the corrections against float64 pow, the ticket
    words, and the update against the host-counter entry at step = t."""
    n, t = 8193, preset + 1
    for hi in (0, 1):
        h, s = ADAM_HYPER[hi], SCALES[hi]
        what = "dev counter %d h%d" % (preset, hi)
        _seed(what)
        p0, m0, v0 = make_state(n)
        g = make_grad(n, m0, f32(h[1]), f32(s))
        nh = RawAdam(p0, m0, v0, h, s).step(g, t, what + " | host")
        ref = check_adam_step(nh, (p0, m0, v0), g, h, t, s, what + " | host")
        dev = RawAdam(p0, m0, v0, h, s, dev=True, counter=preset)
        nd = dev.step(g, t, what + " | dev")
        check_dev_words(dev, t, h, what)
        check_dev_against_host(nd, nh, ref, what)
        check_adam_step(nd, (p0, m0, v0), g, h, t, s, what + " | dev")


# ---- sg_adam_step_dev_multi -------------------------------------------------------------------------------------------------------------------------
MULTI = {          # per set: (n, hyper index, grad_scale, counter preset); a one-workgroup set next to a 2048-workgroup set in two cases
    "2sets": [(3, 0, 1.0, 0), (1048577, 1, 0.125, 9)],
    "3sets": [(8193, 2, 1.0 / 3.0, 999), (3, 3, 1.0, 0), (16385, 0, 0.125, 65535)],
    "4sets": [(16385, 1, 1.0, 1), (3, 0, 1.0 / 3.0, 10 ** 6), (1048577, 2, 1.0, 0), (8193, 3, 0.125, 9)],
}


def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


def multi_call(runs, nsets=None, guard=None, null_at=None):
    """sg_adam_step_dev_multi over RawAdam buffer sets (their G already filled); returns the status"""
    from shapegan_amd.lib import note_device, stream
    lib = _lib()
    addr = lambda get: [None if i == null_at else get(r).view.data_ptr() for i, r in enumerate(runs)]       # noqa: E731
    note_device(runs[0].P.view)
    args = [_arr(ctypes.c_void_p, addr(lambda r: r.P)), _arr(ctypes.c_void_p, addr(lambda r: r.G)), _arr(ctypes.c_void_p, addr(lambda r: r.M)),
            _arr(ctypes.c_void_p, addr(lambda r: r.V)), _arr(ctypes.c_long, [r.n for r in runs])]
    args += [_arr(ctypes.c_float, [r.h[j] for r in runs]) for j in range(3)] + [_arr(ctypes.c_float, [EPS for _ in runs])]
    args += [_arr(ctypes.c_void_p, [r.cnt.view.data_ptr() for r in runs]), _arr(ctypes.c_void_p, [r.corr.view.data_ptr() for r in runs]),
             _arr(ctypes.c_float, [r.s for r in runs])]
    rc = lib.sg_adam_step_dev_multi(len(runs) if nsets is None else nsets, *args, P(guard), stream())
    _sync()
    return rc


def _all_bits(run, what):
    """every word the entry may write, as integers"""
    return [t.view(torch.int32) for t in run.state(what)] + [run.cnt.get(what + " counter"), run.corr.get(what + " corr")]


def _same_all(a, b, what):
    for name, x, y in zip(("p", "m", "v", "counter", "corr and tickets"), a, b):
        assert bool((x == y).all()), "%s: %s differs in bits" % (what, name)


def body_multi(case_id):
    """Two steps of the fused launch: set by set the single-buffer entry's bits (p, m, v, counter, corrections, tickets), and through
    optim.step_together the same."""
    from shapegan_amd import optim
    sets = MULTI[case_id]
    what = "multi " + case_id
    _seed(what)
    states = [make_state(n) for n, _, _, _ in sets]
    fused = [RawAdam(*st, ADAM_HYPER[hi], s, dev=True, counter=c) for st, (n, hi, s, c) in zip(states, sets)]
    single = [RawAdam(*st, ADAM_HYPER[hi], s, dev=True, counter=c) for st, (n, hi, s, c) in zip(states, sets)]
    grads = []
    for k in range(2):
        gs = [make_grad(n, r.M.view.cpu(), f32(r.h[1]), f32(s)) for r, (n, _, s, _) in zip(single, sets)]
        grads.append(gs)
        for r, g in zip(fused, gs):
            r.G.view.copy_(g)
        rc = multi_call(fused)
        assert rc == 0, "%s: returned %d" % (what, rc)
        for i, (r, q, g) in enumerate(zip(fused, single, gs)):
            w = "%s | step %d | set %d" % (what, k, i)
            q.step(g, 0, w)
            r.G.intact(w + " g")
            _same_all(_all_bits(r, w), _all_bits(q, w), w + " (fused against the single-buffer entry)")
            check_dev_words(r, sets[i][3] + k + 1, r.h, w)
    opts = [adam_via_optim(st[0], st[1], st[2], [], ADAM_HYPER[hi], c + 1, s, True)[0] for st, (n, hi, s, c) in zip(states, sets)]
    for gs in grads:
        for o, g in zip(opts, gs):
            o.f.params[0].grad.copy_(g)
        optim.step_together(opts)
    _sync()
    for i, (o, r) in enumerate(zip(opts, fused)):
        n = sets[i][0]
        w = "%s | set %d (optim.step_together against the raw entry)" % (what, i)
        for name, a, b in zip("pmv", (o.f.flat[:n], o.exp_avg[:n], o.exp_avg_sq[:n]), r.state(w)):
            same_bits(a.detach().cpu(), b, w + " | " + name)
        assert int(o.step_dev.cpu()[0]) == sets[i][3] + 2, w


def body_multi_refusals():
    """nsets = 0, nsets = 5 and a null entry are refused as arguments; nothing is written."""
    what = "multi refusals"
    _seed(what)
    runs = [RawAdam(*make_state(n), ADAM_HYPER[i % 4], 1.0, dev=True, counter=3) for i, n in enumerate((513, 3, 8193, 257, 5))]
    for r in runs:
        r.G.view.copy_(torch.randn(r.n))
    before = [_all_bits(r, what) for r in runs]
    for label, sel, nsets, null_at in (("nsets = 0", runs[:1], 0, None), ("nsets = 5", runs, 5, None), ("a null entry", runs[:3], 3, 1),
                                       ("a null last entry", runs[:4], 4, 3)):
        rc = multi_call(sel, nsets=nsets, null_at=null_at)
        assert rc == SG_ERR_ARG, "%s: %s returned %d" % (what, label, rc)
        for r, b in zip(runs, before):
            _same_all(_all_bits(r, what), b, "%s: %s wrote" % (what, label))


def body_guard():
    """With the guard word non-zero sg_adam_step_guarded, sg_adam_step_dev_guarded and the fused launch leave parameters, moments,
    counter, corrections and tickets bit-unchanged; with it cleared the next step is the unguarded step."""
    n, h, s = 8193, ADAM_HYPER[0], 0.125
    what = "guard"
    _seed(what)
    st = make_state(n)
    g = make_grad(n, st[1], f32(h[1]), f32(s))
    for form in ("host", "dev", "multi"):
        w = "%s | %s" % (what, form)
        guard = Words(1, torch.int32, 1)
        mk = lambda gd: [RawAdam(*st, h, s, dev=form != "host", counter=4, guard=gd)] + (             # noqa: E731
            [RawAdam(*make_state(513), ADAM_HYPER[1], 1.0, dev=True, counter=0, guard=gd)] if form == "multi" else [])
        torch.manual_seed(7)
        runs = mk(guard)
        torch.manual_seed(7)
        plain = mk(None)
        g2 = torch.randn(513)

        def go(rs, gd):
            if form == "multi":
                rs[0].G.view.copy_(g)
                rs[1].G.view.copy_(g2)
                assert multi_call(rs, guard=gd) == 0
            else:
                rs[0].step(g, 5, w)
        words = (lambda r: [r.cnt.get(w), r.corr.get(w)]) if form != "host" else (lambda r: [])
        before = [[t.view(torch.int32) for t in r.state(w)] + words(r) for r in runs]
        go(runs, guard)
        for r, b in zip(runs, before):
            for x, y in zip([t.view(torch.int32) for t in r.state(w)] + words(r), b):
                assert bool((x == y).all()), w + ": a guarded step wrote"
        assert int(guard.get(w)[0]) == 1
        guard.view.zero_()
        go(runs, guard)
        go(plain, None)
        for r, q in zip(runs, plain):
            for x, y in zip([t.view(torch.int32) for t in r.state(w)] + words(r), [t.view(torch.int32) for t in q.state(w)] + words(q)):
                assert bool((x == y).all()), w + ": the step after the guard was cleared is not the unguarded step"


# ---- clamps -----------------------------------------------------------------------------------------------------------------------------------------
CLAMP_N = [1, 513, 1048577]
CLAMP_MULTI = [1, 8, 16, 17, 33]
CLAMP_COUNTS = [1, 513, 3, 1100000, 70001, 5, 1024, 2, 16385, 7, 257, 1, 4, 511, 100003, 9, 64]


def clamp_values(n, lo, hi):
    """N(0, 1) at twice the bounds' scale with NaN, +-inf, the bounds themselves, their neighbours and -0 among them"""
    x = torch.randn(n) * 2 * max(abs(lo), abs(hi))
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))       # noqa: E731
    nxt = lambda v, to: float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(to, dtype=torch.float32)))   # noqa: E731
    special = [float("nan"), float("inf"), float("-inf"), f(hi), f(lo), nxt(hi, 9.0), nxt(hi, -9.0), nxt(lo, -9.0), nxt(lo, 9.0), -0.0, 0.0]
    for j, v in enumerate(special):
        if n > len(special):
            x[(j * 47 + n // 3) % n] = v
        elif j < n:
            x[j] = special[(j + n) % len(special)]
    return x


def body_clamp(n):
    from shapegan_amd.lib import check, stream
    lo, hi = -0.3, 0.5
    what = "clamp-%d" % n
    _seed(what)
    x = clamp_values(n, lo, hi)
    if n == 1:
        x[0] = float("nan")
    buf = G32(x)
    check(_lib().sg_clamp(P(buf), n, lo, hi, stream()), what)
    _sync()
    got = buf.get(what)
    same_bits(got, torch.clamp(x, lo, hi), what + " | against torch.clamp")
    assert bool((torch.isnan(got) == torch.isnan(x)).all()) and bool(torch.isnan(x).any()), what + ": a NaN did not survive"


def body_clamp_multi(nt):
    """nt tensors of mixed counts inside ONE arena whose gaps hold NaN: the arena afterwards is torch.clamp of the tensors and the
    gaps' own bits."""
    from shapegan_amd.lib import note_device, check, stream
    lo, hi = -0.01, 0.01
    what = "clamp_multi-%d" % nt
    _seed(what)
    counts = [CLAMP_COUNTS[(i + nt) % len(CLAMP_COUNTS)] for i in range(nt)]
    if nt > 1 and 1100000 not in counts:
        counts[nt // 2] = 1100000
    offs, off = [], 8
    for c in counts:
        offs.append(off)
        off += (c + 3) // 4 * 4 + 4
    arena = torch.full((off + 37,), float("nan"))
    for i, (o, c) in enumerate(zip(offs, counts)):
        arena[o:o + c] = clamp_values(c, lo, hi)
        if c == 1 and i % 2:
            arena[o] = float("nan")
    want = arena.clone()
    for o, c in zip(offs, counts):
        want[o:o + c] = torch.clamp(arena[o:o + c], lo, hi)
    dev = arena.clone().to(OPS.DEV)
    note_device(dev)
    ptrs = (ctypes.c_void_p * nt)(*[dev.data_ptr() + 4 * o for o in offs])
    check(_lib().sg_clamp_multi(ptrs, (ctypes.c_long * nt)(*counts), nt, lo, hi, stream()), what)
    _sync()
    same_bits(dev.cpu(), want, what + " | the arena against torch.clamp of its tensors")
    assert any(bool(torch.isnan(want[o:o + c]).any()) for o, c in zip(offs, counts)), what + ": no NaN among the inputs"


def body_clip_nan():
    """Discriminator.clip_weights and RMSprop(clip = 0.01) with a NaN (and an infinite) weight: the NaN survives, as through the
    reference's p.data.clamp_; everything else is torch.clamp's bits."""
    from shapegan_amd import optim
    from shapegan_amd.model.gan import Discriminator
    torch.manual_seed(15)
    d = Discriminator()
    params = list(d.parameters())
    with torch.no_grad():
        params[0].view(-1)[3] = float("nan")
        params[0].view(-1)[4] = float("inf")
        params[-1].view(-1)[0] = float("nan")
    before = [p.detach().cpu().clone() for p in params]
    d.clip_weights(0.01)
    _sync()
    for i, (p, b) in enumerate(zip(params, before)):
        same_bits(p.detach().cpu(), torch.clamp(b, -0.01, 0.01), "clip_weights_nan | parameter %d against torch.clamp" % i)
    assert bool(torch.isnan(params[0].detach().cpu().view(-1)[3])) and bool(torch.isnan(params[-1].detach().cpu().view(-1)[0]))
    # the clip folded into the RMSprop step
    n = 1000
    p = torch.randn(n) * 0.01
    p[17] = float("nan")
    g = torch.randn(n)
    got = rms_via_optim(p, torch.zeros(n), [g, g], (1e-3, 0.99, 0.01), 1.0)
    assert bool(torch.isnan(got[0][17])), "rmsprop_clip_nan: the NaN weight became %r" % float(got[0][17])
    assert int(torch.isnan(got[0]).sum()) == 1 and float(got[0][~torch.isnan(got[0])].abs().max()) <= f32(0.01)


# ---- sg_reduce_sum ------------------------------------------------------------------------------------------------------------------------------
REDUCE_N = [1, 2, 3, 4, 5, 2047, 2048, 2049, 3145728, 3145732, 3149731, 7344131]


def body_reduce(n):
    """(-1)^i (1000 + N(0, 1)): the sum cancels.  At element offsets 0 - 3 (the kernel tests its own alignment), scale 1 and 1 / n,
    and ops.mean on the same views bit for bit."""
    from shapegan_amd import ops
    from shapegan_amd.lib import check, stream
    lib = _lib()
    what = "reduce-%d" % n
    _seed(what)
    x = (1000.0 + torch.randn(n)) * (1 - 2 * (torch.arange(n) % 2)).float()
    total, sumabs = float(x.double().sum()), float(x.double().abs().sum())
    for off in range(4):
        gx = Guarded((n,), x, off=8 + off)
        for scale in (1.0, 1.0 / n):
            w = "%s | offset %d | scale %.3g" % (what, off, scale)
            out = G32(torch.full((1,), float("nan")))
            ws = Workspace(lib.sg_reduce_workspace_bytes())
            check(lib.sg_reduce_sum(P(gx), P(out), n, scale, ws.ptr(), ws.nbytes, stream()), w)
            _sync()
            ws.check(w)
            got = out.get(w)
            ref = total * f32(scale)
            bound = U * abs(ref) + n * 2.0 ** -53 * sumabs * f32(scale)
            check_bound(got, torch.tensor([ref], dtype=torch.float64), torch.tensor([bound], dtype=torch.float64), w, "reduce")
        via = ops.mean(gx.view)
        _sync()
        same_bits(via.detach().cpu().reshape(1), got, what + " | offset %d | ops.mean against the raw entry" % off)
        gx.intact(what + " x")


# ---- activations ------------------------------------------------------------------------------------------------------------------------------------
ACTS = [(NONE, 0.0), (LEAKY, 0.2), (LEAKY, 0.01), (RELU, 0.0), (TANH, 0.0), (SIGMOID, 0.0)]
ACT_N = [1, 2, 3, 4, 5, 7, 1023, 1025, 2097155]
ROWSUM_S = [1, 3, 4, 64, 255, 1021, 1024, 1028, 32768]
ACT_SPECIAL = [0.0, 100.0, -100.0, -0.0, 88.8, -88.8, 20.0, -20.0, 1e-6, -1e-6, 103.0 * 0.5, -17.0, 0.5, -0.5]


def act_inputs(n):
    x = (torch.randn(n) * 30).clamp(-100, 100)
    for i in range(min(n, len(ACT_SPECIAL))):
        x[i] = ACT_SPECIAL[(i + n) % len(ACT_SPECIAL)]
    return x, torch.randn(n)


def act64(x, act, slope):
    x = x.double()
    if act in (LEAKY, RELU):
        return torch.where(x > 0, x, x * (slope if act == LEAKY else 0.0))
    return {NONE: lambda t: t, TANH: torch.tanh, SIGMOID: torch.sigmoid}[act](x)


def act_bwd64(y, dy, act, slope):
    """dx from the fp32 y the kernel is given, and the magnitude of its bound (to be multiplied by u)"""
    y, dy = y.double(), dy.double()
    if act == TANH:
        return dy * (1 - y * y), K_ACT * dy.abs() * (1 + y * y)
    if act == SIGMOID:
        return dy * y * (1 - y), K_ACT * dy.abs() * (y.abs() + y * y)
    if act in (LEAKY, RELU):
        return torch.where(y > 0, dy, dy * (slope if act == LEAKY else 0.0)), 2 * dy.abs()
    return dy, 2 * dy.abs()


def body_act(n):
    from shapegan_amd import ops
    from shapegan_amd.lib import check, stream
    lib = _lib()
    for act, slope in ACTS:
        what = "act-%d | act %d slope %g" % (n, act, slope)
        _seed(what)
        x, dy = act_inputs(n)
        gx, gy = G32(x), G32(torch.full((n,), float("nan")))
        check(lib.sg_act_fwd(P(gx), P(gy), n, act, slope, stream()), what)
        _sync()
        y = gy.get(what + " y")
        ref = act64(x, act, f32(slope))
        check_bound(y, ref, K_ACT * U * ref.abs() + FLT_MIN, what, "act.fwd")
        gdy, gdx = G32(dy), G32(torch.full((n,), float("nan")))
        check(lib.sg_act_bwd(P(gy), P(gdy), P(gdx), n, act, slope, stream()), what)
        _sync()
        dx = gdx.get(what + " dx")
        dref, mag = act_bwd64(y, dy, act, f32(slope))
        check_bound(dx, dref, U * mag + DENORM_FLOOR, what, "act.bwd")
        for g in (gx, gy, gdy):
            g.intact(what + " (an input)")
        xv = gx.view.detach().requires_grad_(True)
        yv = ops.Act.apply(xv, act, slope)
        yv.backward(gdy.view)
        _sync()
        same_bits(yv.detach().cpu(), y, what + " | y (ops.Act against the raw entry)")
        same_bits(xv.grad.cpu(), dx, what + " | dx (ops.Act against the raw entry)")


def body_act_rowsum(S):
    from shapegan_amd import ops
    from shapegan_amd.lib import check, stream
    lib = _lib()
    for rows in (1, 5):
        for act, slope in (ACTS[(ROWSUM_S.index(S) + rows) % len(ACTS)], ACTS[(ROWSUM_S.index(S) + rows + 3) % len(ACTS)]):
            what = "act_rowsum-%dx%d | act %d slope %g" % (rows, S, act, slope)
            _seed(what)
            x, dy = act_inputs(rows * S)
            y = act64(x / 10, act, f32(slope)).float()            # (any fp32 y is a legal input; x / 10 leaves tanh and sigmoid a slope)
            gy, gdy = G32(y), G32(dy)
            gdx, gdx2, gsum = (G32(torch.full((k,), float("nan"))) for k in (rows * S, rows * S, rows))
            check(lib.sg_act_bwd_rowsum(P(gy), P(gdy), P(gdx), P(gsum), rows, S, act, slope, stream()), what)
            check(lib.sg_act_bwd(P(gy), P(gdy), P(gdx2), rows * S, act, slope, stream()), what)
            _sync()
            dx, sums = gdx.get(what + " dx"), gsum.get(what + " rowsum")
            same_bits(dx, gdx2.get(what), what + " | dx of act_bwd_rowsum against act_bwd")
            dref, mag = act_bwd64(y, dy, act, f32(slope))
            check_bound(dx, dref, U * mag, what, "act.bwd")
            dref = dref.view(rows, S)
            check_bound(sums, dref.sum(1), K_ACT * U * dref.abs().sum(1), what, "act.rowsum")
            for g in (gy, gdy):
                g.intact(what + " (an input)")
            dz, _ = ops.act_bwd_rowsum_raw(gy.view.view(rows, 1, S), gdy.view.view(rows, 1, S), act, slope)
            _sync()
            same_bits(dz.cpu().reshape(-1), dx, what + " | dz (ops.act_bwd_rowsum_raw against the raw entry)")


# ---- latent-table rows ------------------------------------------------------------------------------------------------------------------------------
ROWS_L = [1, 3, 128, 130]
ROWS_N = [1, 1000, 9000]          # 9000 x 130 and 9000 x 128 are past one grid-stride round of 2048 x 512 elements
TABLE_ROWS = 37


def body_rows(L):
    from shapegan_amd import ops
    from shapegan_amd.lib import check, stream
    lib = _lib()
    R = TABLE_ROWS
    for n in ROWS_N:
        for dist in ("uniform", "equal", "hot"):
            what = "rows L=%d n=%d %s" % (L, n, dist)
            _seed(what)
            idx = torch.randint(0, R, (n,))
            if dist == "equal":
                idx[:] = 5
            elif dist == "hot":
                idx[torch.rand(n) < 0.5] = 3
            table, g = torch.randn(R, L), torch.randn(n, L)
            gt, gi = Guarded((R, L), table, off=8), _dev(idx)
            gout = G32(torch.full((n * L,), float("nan")))
            check(lib.sg_gather_rows(P(gt), ops.ptr(gi), P(gout), n, L, stream()), what)
            _sync()
            rows = gout.get(what + " out")
            same_bits(rows.view(n, L), table[idx], what + " | gather against table[idx]")
            gt.intact(what + " table")
            tg = gt.view.detach().requires_grad_(True)
            via = ops.gather_rows(tg, gi)
            same_bits(via.detach().cpu(), rows.view(n, L), what + " | ops.gather_rows against the raw entry")
            count = torch.bincount(idx, minlength=R).double()
            ref = torch.zeros(R, L, dtype=torch.float64).index_add_(0, idx, g.double())
            bound = (count - 1).clamp(min=0)[:, None] * U * torch.zeros(R, L, dtype=torch.float64).index_add_(0, idx, g.double().abs())
            for ld in (L, L + 5):
                w = "%s ld=%d" % (what, ld)
                padded = torch.full((n, ld), float("nan"))
                padded[:, :L] = g
                grows = G32(padded.reshape(-1))
                gtab = G32(torch.zeros(R * L))
                check(lib.sg_scatter_add_rows(P(grows), ld, ops.ptr(gi), P(gtab), n, L, stream()), w)
                _sync()
                check_bound(gtab.get(w + " table_grad"), ref, bound, w + " | raw", "scatter")
                grows.intact(w + " rows")
                if tg.grad is not None:
                    tg.grad = None
                via.backward(grows.view.view(n, ld)[:, :L], retain_graph=True)
                _sync()
                check_bound(tg.grad.cpu(), ref, bound, w + " | ops.gather_rows backward", "scatter")


# ---- sg_axpby ---------------------------------------------------------------------------------------------------------------------------------------
AXPBY_N = [1, 513, 1048577]


def body_axpby(n):
    from shapegan_amd.lib import check, stream
    lib = _lib()
    for a, b in ((1.0, 1.0), (0.3, -0.7), (1.0, 0.0)):
        for with_y in (True, False):
            what = "axpby-%d a=%g b=%g y=%s" % (n, a, b, with_y)
            _seed(what)
            x, y = torch.randn(n), torch.randn(n) * 3
            gx, gy, gout = G32(x), (G32(y) if with_y else None), G32(torch.full((n,), float("nan")))
            check(lib.sg_axpby(P(gx), P(gy), P(gout), n, a, b, stream()), what)
            _sync()
            ax, by = f32(a) * x.double(), (f32(b) * y.double() if with_y else torch.zeros(n, dtype=torch.float64))
            check_bound(gout.get(what + " out"), ax + by, 2 * U * (ax.abs() + by.abs()), what, "axpby")
            gx.intact(what + " x")


# ---- calibration (not a test: run by hand on the CPU) ---------------------------------------------------------------------------------------------------
def _ratio(got, want, mag):
    err = (got.double() - want.double()).abs().reshape(-1)
    r = torch.where(err == 0, torch.zeros_like(err), err / (U * mag.double().reshape(-1)))
    return float(r.max()) if r.numel() else 0.0


def torch_fp32_ratios():
    """The largest ratio of torch's own fp32 CPU optimizers and activations against the bounds above with K = K_ACT = 1, over the table."""
    worst = {}

    def note(key, val, what):
        if val > worst.get(key, 0.0):
            worst[key] = val
            print("[optim-forms] torch fp32 | %s | %s | %.3g" % (what, key, val))
    for n in ALL_N:
        for hi, s, t0, steps in adam_cases(n):
            h = ADAM_HYPER[hi]
            what = "adam n=%d (%d wg) h%d s%.3g t0=%d" % (n, workgroups(n), hi, s, t0)
            _seed(what)
            st = make_state(n)
            for k in range(steps):
                g = make_grad(n, st[1], f32(h[1]), f32(s))
                lr, b1, b2 = _h32(h)
                ref = adam_formula(st[0], g, st[1], st[2], lr, b1, b2, f32(EPS), t0 + k, f32(s))
                st = torch_adam_step(st[0], g, st[1], st[2], h, t0 + k, s)
                for name, got in zip("pmv", st):
                    note("adam." + name, _ratio(got, ref[name], ref[name + "_mag"]), what)
        for ri, s, steps in rms_cases(n):
            r = RMS_HYPER[ri]
            what = "rmsprop n=%d (%d wg) lr=%g alpha=%g clip=%g s%.3g" % (n, workgroups(n), r[0], r[1], r[2], s)
            _seed(what)
            p, _, sq = make_state(n, r[2])
            for k in range(steps):
                g = make_grad(n, None, 0.0, f32(s))
                lr, alpha, clip = _h32(r)
                ref = rms_formula(p, g, sq, lr, alpha, f32(EPS), f32(s), clip)
                p, sq = torch_rms_step(p, g, sq, r, s)
                note("rms.p", _ratio(p, ref["p"], ref["p_mag"]), what)
                note("rms.sq", _ratio(sq, ref["sq"], ref["sq_mag"]), what)
    fns = {NONE: lambda t, s: t * 1, LEAKY: F.leaky_relu, RELU: lambda t, s: torch.relu(t), TANH: lambda t, s: torch.tanh(t),
           SIGMOID: lambda t, s: torch.sigmoid(t)}
    for n in ACT_N + [5 * S for S in ROWSUM_S]:
        for act, slope in ACTS:
            what = "act-%d | act %d slope %g" % (n, act, slope)
            _seed(what)
            x, dy = act_inputs(n)
            xt = x.clone().requires_grad_(True)
            y = fns[act](xt, slope)
            y.backward(dy)
            ref = act64(x, act, f32(slope))
            note("act.fwd", float(((y.detach().double() - ref).abs() / (U * ref.abs() + FLT_MIN)).max()), what)
            dref, mag = act_bwd64(y.detach(), dy, act, f32(slope))
            note("act.bwd", _ratio(xt.grad, dref, mag / (K_ACT if act in (TANH, SIGMOID) else 1.0) + DENORM_FLOOR / U), what)
            if n % 5 == 0 and n // 5 in ROWSUM_S:
                note("act.rowsum", _ratio(xt.grad.view(5, -1).sum(1), dref.view(5, -1).sum(1), dref.view(5, -1).abs().sum(1)), what)
    return worst
