"""Device-neutral bodies of the t-SNE tests (K17: csrc/tsne.hip, its twin, shapegan_amd/traversal.py tsne).  tests/test_tsne.py runs them
on the C++ twin, tests/test_gpu_tsne.py on the GPU.

Criterion (test_gpu_modules.check_against_oracles at its defaults), against the restatements of tests/tsne_reference.py:
    |got - ref64| <= 1e-4 * mean|ref64| + 4 * max|ref32 - ref64|
Affinities are compared at tol = 0, so that the implementation and both restatements run the search to its root instead of stopping
at different steps.  Every check records its worst err / tol in WORST (printed by the tests with -s).

Inputs are seeded Gaussian clusters with two coincident rows (0 and 1) and one far outlier (the last row); the embeddings are seeded
normal draws at scale 1e-4 (the start of an optimisation) and 5 (late).  Sizes: every N on each side of a tile edge of the kernels —
the 64-wide distance tile, the 32-wide symmetrisation tile, the 256 lanes of a row search and of a gradient workgroup, the 4 rows of a
gradient workgroup and its float4 path (N a multiple of 4), whose lanes cover 1024 columns per load (1028); a gradient workgroup
flushes its float sums into float64 every 4096 columns, so 4100 (float4 path) and 4101 (dword path) take a second pass — there on a
synthetic symmetric P, which is all the gradient kernels see."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_modules as M
import tsne_reference as R
from shapegan_amd import lib as L
from shapegan_amd import ops
from shapegan_amd import traversal as T

SIZES = (4, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 1028)
DIMS = (1, 3, 128, 131)
AFFINITY_CASES = [(n, 3) for n in SIZES] + [(n, d) for n in (65, 300) for d in DIMS if d != 3]
WORST = {}


def perplexity_for(n):
    return 2.5 if n == 4 else min(30.0, n / 4.0)      # (N = 4: rows 0 and 1 coincide, so the outlier's entropy cannot go below log 2)


@functools.lru_cache(maxsize=None)
def points(n, d):
    x = R.clusters(n, d, 3, 100 + n + d)
    x[1] = x[0]
    x[-1] = x[-1] + 50.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference_affinities(n, d, precision):
    out = R.affinities(points(n, d), perplexity_for(n), tol=0.0, max_steps=100, dtype=np.float64 if precision == 64 else np.float32)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


def embedding(n, scale, seed=7):
    return (np.random.RandomState(seed + n).randn(n, 2) * scale).astype(np.float32)


def note(body, what, ratio):
    key = (body, what)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("%s: %s: worst err / tol %.3f" % (body, what, ratio))


def check(body, got, ref32, ref64, what):
    g = torch.as_tensor(np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)).reshape(-1)
    r32 = torch.as_tensor(np.asarray(ref32, dtype=np.float64)).reshape(-1)
    r64 = torch.as_tensor(np.asarray(ref64, dtype=np.float64)).reshape(-1)
    assert g.shape == r64.shape, "%s: %d elements, reference %d" % (what, g.numel(), r64.numel())
    tol = M.RTOL * float(r64.abs().mean()) + 4.0 * float((r32 - r64).abs().max())
    note(body, what, float((g - r64).abs().max()) / tol)
    M.check_against_oracles(g, r32, r64, what)


def t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


# ---- affinities -----------------------------------------------------------------------------------------------------------------------
def body_affinities(dev, n, d):
    P, beta, plogp = ops.tsne_affinities(t(points(n, d), dev), perplexity_for(n), tol=0.0, max_steps=100)
    P64, b64, l64 = reference_affinities(n, d, 64)
    P32, b32, l32 = reference_affinities(n, d, 32)
    what = "N=%d D=%d" % (n, d)
    check("affinities", P, P32, P64, what + " P")
    check("affinities", beta, b32, b64, what + " beta")
    check("affinities", plogp, [l32], [l64], what + " plogp")
    P = P.cpu()
    assert torch.equal(P, P.t()), what + ": P is not exactly symmetric"
    assert float(P.diagonal().abs().max()) == 0.0, what + ": the diagonal is not exactly zero"
    assert bool((P >= 0).all())
    assert abs(float(P.double().sum()) - 1.0) <= n * n * 2.0 ** -24, what + ": sum P = %r" % float(P.double().sum())


def body_entropy(dev, n, d):
    """At the default tol = 1e-5 every row's search ends within tol of log(perplexity).  The symmetrised P no longer holds a row's
    conditional distribution, so the entropy is recomputed in float64 from the float64 distances and the returned beta; the noise
    term is what the float32 restatement's evaluation of the entropy at that same beta differs from the float64 one by."""
    x = points(n, d)
    _, beta, _ = ops.tsne_affinities(t(x, dev), perplexity_for(n), tol=1e-5, max_steps=100)
    beta = beta.cpu().numpy()
    h64 = R.row_entropy_at(x, beta, np.float64)
    h32 = R.row_entropy_at(x, beta, np.float32)
    tol = 1e-5 + 4.0 * float(np.abs(h32 - h64).max())
    err = float(np.abs(h64 - np.log(perplexity_for(n))).max())
    note("entropy", "N=%d D=%d" % (n, d), err / tol)
    assert err <= tol, "N=%d D=%d: a row's entropy is %.3e from log(perplexity), tol %.3e" % (n, d, err, tol)


def body_sklearn(dev, n=300, d=3):
    """Against scikit-learn's own _joint_probabilities (which stops its search at 1e-5): within the criterion plus what the float64
    restatement itself differs from scikit-learn by."""
    pytest.importorskip("sklearn")
    from sklearn.manifold._t_sne import _joint_probabilities
    from scipy.spatial.distance import squareform
    x = points(n, d)
    sk = squareform(_joint_probabilities(R.distances(x, np.float64).astype(np.float32), perplexity_for(n), 0))
    P, _, _ = ops.tsne_affinities(t(x, dev), perplexity_for(n), tol=0.0, max_steps=100)
    P64, P32 = reference_affinities(n, d, 64)[0], reference_affinities(n, d, 32)[0]
    tol = M.RTOL * float(np.abs(sk).mean()) + 4.0 * float(np.abs(P32 - P64).max()) + float(np.abs(P64 - sk).max())
    err = float(np.abs(P.cpu().numpy().astype(np.float64) - sk).max())
    note("sklearn", "N=%d" % n, err / tol)
    assert err <= tol, (err, tol)


# ---- gradient and kl ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def joint(n):
    P = reference_affinities(n, 3, 64)[0].astype(np.float32)
    P.setflags(write=False)
    return P, R.plogp(P)


def body_gradient(dev, n, scale, exaggeration):
    P, lp = joint(n)
    y = embedding(n, scale)
    g64, k64 = R.gradient(y, P, exaggeration, lp, np.float64)
    g32, k32 = R.gradient(y, P, exaggeration, lp, np.float32)
    grad, kl = ops.tsne_gradient(t(y, dev), t(P, dev), exaggeration, torch.tensor([lp], dtype=torch.float64, device=dev))
    what = "N=%d scale=%g exaggeration=%g" % (n, scale, exaggeration)
    check("gradient", grad, g32, g64, what + " grad")
    check("gradient", kl, [k32], [k64], what + " kl")
    alone = ops.tsne_gradient(t(y, dev), t(P, dev), exaggeration)
    assert torch.equal(alone, grad), what + ": the gradient without kl differs from the one with it"


LARGE = (4100, 4101)


@functools.lru_cache(maxsize=None)
def synthetic_joint(n):
    a = np.random.RandomState(n).rand(n, n).astype(np.float32)
    a = a + a.T
    np.fill_diagonal(a, 0)
    P = (a / a.sum(dtype=np.float64)).astype(np.float32)
    P.setflags(write=False)
    return P, R.plogp(P)


def body_gradient_large(dev, n):
    """More columns than one pass of a gradient workgroup covers: the float64 accumulators are added to a second time.  The reference
    gradient is taken on 96 rows (the first and last workgroups' and seeded others); Z and kl take every pair."""
    P, lp = synthetic_joint(n)
    y = embedding(n, 5.0)
    rows = np.unique(np.concatenate([np.arange(8), np.arange(n - 8, n), np.random.RandomState(n).randint(0, n, 80)]))
    g64, k64 = R.gradient(y, P, 1.0, lp, np.float64, rows=rows)
    g32, k32 = R.gradient(y, P, 1.0, lp, np.float32, rows=rows)
    grad, kl = ops.tsne_gradient(t(y, dev), t(P, dev), 1.0, torch.tensor([lp], dtype=torch.float64, device=dev))
    assert bool(torch.isfinite(grad).all())
    check("gradient", grad.cpu()[torch.from_numpy(rows)], g32, g64, "N=%d grad" % n)
    check("gradient", kl, [k32], [k64], "N=%d kl" % n)


def body_finite_difference():
    """Pins the definition: in the float64 restatement, grad at exaggeration 1 is the derivative of kl."""
    n = 65
    P, lp = joint(n)
    y = embedding(n, 1.0).astype(np.float64)
    g, _ = R.gradient(y, P, 1.0, lp)
    rng = np.random.RandomState(3)
    for _ in range(4):
        v = rng.randn(n, 2)
        h = 1e-5
        fd = (R.gradient(y + h * v, P, 1.0, lp)[1] - R.gradient(y - h * v, P, 1.0, lp)[1]) / (2 * h)
        assert abs(fd - float((g * v).sum())) <= 1e-6 * max(1.0, abs(fd)), (fd, float((g * v).sum()))


# ---- lockstep optimisation ------------------------------------------------------------------------------------------------------------
LOCK_N, LOCK_STEPS, LOCK_SWITCH, FRAGILE_CAP = 300, 120, 60, 1e-3


@functools.lru_cache(maxsize=None)
def lockstep_problem():
    x = R.clusters(LOCK_N, 16, 5, 0)
    P = R.affinities(x, 30.0, tol=1e-5, max_steps=100, dtype=np.float64)[0].astype(np.float32)
    y0 = (np.random.RandomState(1).randn(LOCK_N, 2) * 1e-4).astype(np.float32)
    return P, y0


def body_lockstep(dev):
    """120 steps at N = 300, the switch from exaggeration 12 / momentum 0.5 to 1 / 0.8 at step 60.  Before every step the float64 and
    float32 restatements recompute gradient and update from the implementation's own state; grad, velocity, gains and Y are held to
    the criterion.  The gains rule is a sign decision: an element whose |grad_ref64| is within the criterion's tolerance of zero at a
    step may take either branch and is left out of velocity, gains and Y at that step; such element-steps stay under FRAGILE_CAP."""
    P, y0 = lockstep_problem()
    Pd = t(P, dev)
    y, vel, gains = t(y0, dev).clone(), torch.zeros(LOCK_N, 2, device=dev), torch.ones(LOCK_N, 2, device=dev)
    lr = T.auto_learning_rate(LOCK_N, 12.0)
    fragile, total = 0, 0
    worst = {"grad": 0.0, "velocity": 0.0, "gains": 0.0, "Y": 0.0}
    for it in range(LOCK_STEPS):
        ex, mom = (12.0, 0.5) if it < LOCK_SWITCH else (1.0, 0.8)
        state = [a.cpu().numpy().copy() for a in (y, vel, gains)]
        grad = ops.tsne_step(y, Pd, vel, gains, ex, mom, lr)
        refs = {}
        for name, dt in (("64", np.float64), ("32", np.float32)):
            g, _ = R.gradient(state[0], P, ex, 0.0, dt)
            refs[name] = (g,) + R.update(state[0], state[1], state[2], g, mom, lr, dtype=dt)
        g64, g32 = refs["64"][0], refs["32"][0]
        gtol = M.RTOL * float(np.abs(g64).mean()) + 4.0 * float(np.abs(g32 - g64).max())
        safe = np.abs(g64) > gtol
        fragile += int((~safe).sum())
        total += safe.size
        got = dict(grad=grad, Y=y, velocity=vel, gains=gains)
        for k, name in enumerate(("grad", "Y", "velocity", "gains")):
            g = got[name].cpu().numpy().astype(np.float64)
            r64, r32 = refs["64"][k].astype(np.float64), refs["32"][k].astype(np.float64)
            tol = M.RTOL * float(np.abs(r64).mean()) + 4.0 * float(np.abs(r32 - r64).max())
            keep = np.ones_like(safe) if name == "grad" else safe
            err = float(np.abs(g - r64)[keep].max())
            worst[name] = max(worst[name], err / tol)
            assert err <= tol, "step %d %s: err %.3e tol %.3e" % (it, name, err, tol)
    for name, ratio in worst.items():
        note("lockstep", name, ratio)
    print("lockstep: fragile element-steps %d of %d = %.2e" % (fragile, total, fragile / total))
    assert fragile <= FRAGILE_CAP * total, "fragile element-steps: %d of %d" % (fragile, total)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
E2E_SEEDS = (1, 2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def end_to_end_reference():
    """Final KL of the float64 restatement from five seeded inits (N = 300, D = 16, 5 clusters, perplexity 30, 1000 iterations)."""
    x = R.clusters(300, 16, 5, 0)
    P = R.affinities(x, 30.0, tol=1e-5, max_steps=100, dtype=np.float64)[0]
    return tuple(R.run(P, np.random.RandomState(s).randn(300, 2) * 1e-4)[1] for s in E2E_SEEDS)


@functools.lru_cache(maxsize=None)
def end_to_end_sklearn():
    from sklearn.manifold import TSNE
    x = R.clusters(300, 16, 5, 0)
    return tuple(float(TSNE(method="exact", init="random", random_state=s, perplexity=30.0).fit(x).kl_divergence_) for s in E2E_SEEDS)


def body_end_to_end(dev, against="restatement"):
    if against == "sklearn":
        pytest.importorskip("sklearn")
    kls = end_to_end_reference() if against == "restatement" else end_to_end_sklearn()
    x = R.clusters(300, 16, 5, 0)
    y0 = torch.from_numpy((np.random.RandomState(E2E_SEEDS[0]).randn(300, 2) * 1e-4).astype(np.float32))
    y, kl = T.tsne(t(x, dev), perplexity=30, iterations=1000, init=y0, return_kl=True)
    bound = max(kls) + (max(kls) - min(kls))
    print("end to end (%s): kl %.5f, reference runs %.5f .. %.5f, bound %.5f" % (against, kl, min(kls), max(kls), bound))
    assert y.shape == (300, 2) and y.device.type == torch.device(dev).type and bool(torch.isfinite(y).all())
    assert kl <= bound, "final kl %.5f beyond %.5f (reference runs %s)" % (kl, bound, kls)


# ---- identities -----------------------------------------------------------------------------------------------------------------------
def body_repeat(dev, n=257):
    x, (P, lp), y = t(points(n, 3), dev), joint(n), embedding(n, 5.0)
    a, b = ops.tsne_affinities(x, perplexity_for(n)), ops.tsne_affinities(x, perplexity_for(n))
    assert all(torch.equal(u, v) for u, v in zip(a, b)), "two affinity calls differ"
    lpt = torch.tensor([lp], dtype=torch.float64, device=dev)
    g1, g2 = ops.tsne_gradient(t(y, dev), t(P, dev), 12.0, lpt), ops.tsne_gradient(t(y, dev), t(P, dev), 12.0, lpt)
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1]), "two gradient calls differ"


def body_step_is_gradient_then_update(dev, n):
    P, lp = joint(n)
    Pd, lpt = t(P, dev), torch.tensor([lp], dtype=torch.float64, device=dev)
    rng = np.random.RandomState(11)
    start = [t(embedding(n, 2.0), dev), t((rng.randn(n, 2) * 0.1).astype(np.float32), dev), t((0.5 + rng.rand(n, 2)).astype(np.float32), dev)]
    a = [s.clone() for s in start]
    ga, ka = ops.tsne_step(a[0], Pd, a[1], a[2], 12.0, 0.5, 50.0, plogp=lpt)
    b = [s.clone() for s in start]
    gb, kb = ops.tsne_gradient(b[0], Pd, 12.0, lpt)
    ops.tsne_update(b[0], b[1], b[2], gb, 0.5, 50.0)
    assert torch.equal(ga, gb) and torch.equal(ka, kb)
    for u, v, s, name in zip(a, b, start, ("Y", "velocity", "gains")):
        assert torch.equal(u, v), name + ": sg_tsne_step differs from gradient + update"
        assert not torch.equal(u, s), name + " did not move"


def body_permutation(dev, n=65, d=3):
    """Permuting the rows of X permutes P.  The squared distances are permuted bit for bit, but a row's sums are added in column
    order, so the permuted search sees other last bits: the identity holds WITHIN THE CRITERION, not exactly."""
    x = points(n, d)
    perm = np.random.RandomState(5).permutation(n)
    P, _, _ = ops.tsne_affinities(t(x, dev), perplexity_for(n), tol=0.0)
    Pp, _, _ = ops.tsne_affinities(t(x[perm], dev), perplexity_for(n), tol=0.0)
    P64, P32 = reference_affinities(n, d, 64)[0], reference_affinities(n, d, 32)[0]
    check("permutation", Pp, P32[np.ix_(perm, perm)], P64[np.ix_(perm, perm)], "N=%d" % n)
    tol = M.RTOL * float(np.abs(P64).mean()) + 4.0 * float(np.abs(P32 - P64).max())
    assert float((Pp.cpu() - P.cpu()[perm][:, perm]).abs().max()) <= 2 * tol


def body_inits_and_learning_rate(dev):
    assert T.auto_learning_rate(300, 12) == 50.0 and T.auto_learning_rate(9600, 12) == 200.0
    x = t(R.clusters(80, 6, 3, 2), dev)
    pca = T.tsne(x, perplexity=10, iterations=0)
    assert pca.shape == (80, 2) and pca.dtype == torch.float32 and pca.device.type == torch.device(dev).type
    assert torch.equal(pca.cpu(), T.pca_init(x).float())
    assert abs(float(pca[:, 0].double().std(unbiased=False)) - 1e-4) < 1e-9
    c = x.double().cpu() - x.double().cpu().mean(dim=0)
    _, _, vt = torch.linalg.svd(c, full_matrices=False)
    for k in range(2):      # the documented sign: the loading of largest magnitude is positive
        lead = vt[k] * torch.sign(vt[k][vt[k].abs().argmax()])
        assert torch.allclose((c @ lead) / (c @ vt[0]).std(unbiased=False) * 1e-4, pca[:, k].double().cpu(), atol=1e-9)
    r0, r0b, r1 = (T.tsne(x, perplexity=10, iterations=0, init="random", seed=s) for s in (0, 0, 1))
    assert torch.equal(r0, r0b) and not torch.equal(r0, r1) and 5e-5 < float(r0.std()) < 2e-4
    given = torch.randn(80, 2, generator=torch.Generator().manual_seed(4))
    assert torch.equal(T.tsne(x, perplexity=10, iterations=0, init=given).cpu(), given)
    auto = T.tsne(x, perplexity=10, iterations=5, exaggeration_iterations=3, init=given)
    fixed = T.tsne(x, perplexity=10, iterations=5, exaggeration_iterations=3, init=given, lr=50.0)
    other = T.tsne(x, perplexity=10, iterations=5, exaggeration_iterations=3, init=given, lr=80.0)
    assert torch.equal(auto, fixed) and not torch.equal(auto, other)
    with pytest.raises(ValueError):
        T.tsne(x, init="spectral")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def body_refusals(dev):
    """Through the raw ABI of the library that serves `dev`: refused with a non-zero code before any launch — nothing is written."""
    cuda = torch.device(dev).type == "cuda"
    lib = L._load_hip() if cuda else L.load_cpu()
    suffix = "" if cuda else "_cpu"
    stream = torch.cuda.current_stream().cuda_stream if cuda else None
    n = 8
    x = torch.randn(n, 3, device=dev)
    P = torch.full((n, n), 7.0, device=dev)
    beta = torch.full((n,), 7.0, device=dev)
    plogp = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    ws = torch.full((64 * n,), 7.0, dtype=torch.float64, device=dev)
    nbytes = ws.numel() * 8
    aff = getattr(lib, "sg_tsne_affinities" + suffix)

    def affinities(N, D, perplexity, ws_bytes=nbytes, tol=1e-5, steps=100):
        return aff(x.data_ptr(), N, D, perplexity, tol, steps, P.data_ptr(), beta.data_ptr(), plogp.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    assert affinities(n, 3, 2.0) == 0      # the same call with good arguments is accepted
    P.fill_(7.0), beta.fill_(7.0), plogp.fill_(7.0), ws.fill_(7.0)
    assert affinities(3, 3, 1.0) != 0, "N = 3 accepted"
    assert affinities(n, 0, 2.0) != 0, "D = 0 accepted"
    assert affinities(n, 3, float(n - 1)) != 0, "perplexity = N - 1 accepted"
    assert affinities(n, 3, 0.5) != 0, "perplexity < 1 accepted"
    assert affinities(ops.TSNE_MAX_POINTS + 1, 3, 30.0) != 0, "N over the limit accepted"
    assert affinities(n, 3, 2.0, ws_bytes=8 * n - 1) != 0, "a short workspace accepted"
    assert affinities(n, 3, 2.0, steps=0) != 0 and affinities(n, 3, 2.0, tol=-1.0) != 0
    y = torch.randn(n, 2, device=dev)
    state = [torch.full((n, 2), 7.0, device=dev) for _ in range(3)]      # grad, velocity, gains
    grad_fn, step_fn = getattr(lib, "sg_tsne_gradient" + suffix), getattr(lib, "sg_tsne_step" + suffix)
    y_before = y.clone()
    for N, ws_bytes in ((3, nbytes), (ops.TSNE_MAX_POINTS + 1, nbytes), (n, 8 * (6 * n + 2) - 1)):
        assert grad_fn(y.data_ptr(), P.data_ptr(), N, 1.0, None, state[0].data_ptr(), None, ws.data_ptr(), ws_bytes, stream) != 0
        assert step_fn(y.data_ptr(), P.data_ptr(), N, 1.0, None, state[1].data_ptr(), state[2].data_ptr(), 0.5, 50.0, 0.01,
                       state[0].data_ptr(), None, ws.data_ptr(), ws_bytes, stream) != 0
    if cuda:
        torch.cuda.synchronize()
    for buf in [P, beta, plogp, ws] + state:
        assert bool((buf == 7.0).all()), "a refused call wrote something"
    assert torch.equal(y, y_before)
    with pytest.raises(RuntimeError):
        ops.tsne_affinities(x, perplexity=float(n))
