"""Exact t-SNE restated in numpy from the definitions of include/shapegan_hip.h, K17, in float64 and in float32.

`dtype` is the precision of the per-element arithmetic (differences, exp, the weights of a pair, the update); the sums the header
defines as float64 (a row's sum_p / sum_dp, the sums of a gradient row, Z, plogp, kl) are float64 in both.  The float32 restatement is
what an implementation in the header's precision can be expected to give: |ref32 - ref64| is the noise term of the tests' criterion.
Nothing here is shared with the code under test."""
import numpy as np


def clusters(n, d, k, seed):
    """n seeded points in d dimensions around k Gaussian centres (float32)."""
    r = np.random.RandomState(seed)
    c = r.randn(k, d) * 4
    return (c[r.randint(0, k, n)] + r.randn(n, d)).astype(np.float32)


def distances(X, dtype):
    X = X.astype(dtype)
    diff = X[:, None, :] - X[None, :, :]
    return (diff * diff).sum(axis=2, dtype=dtype)


def entropies(D2, beta, dtype):
    """Per row i: (H_i, sum_p, p [N, N] unnormalised with a zero diagonal) at beta_i, on distances shifted by the row's off-diagonal
    minimum."""
    n = D2.shape[0]
    off = ~np.eye(n, dtype=bool)
    m = np.where(off, D2, np.inf).min(axis=1)
    d = np.where(off, D2 - m[:, None], 0).astype(dtype)
    p = np.exp(-beta.astype(dtype)[:, None] * d).astype(dtype)
    p[~off] = 0
    sum_p = p.sum(axis=1, dtype=np.float64)
    sum_dp = (d.astype(np.float64) * p.astype(np.float64) * off).sum(axis=1)
    return np.log(sum_p) + beta.astype(np.float64) * sum_dp / sum_p, sum_p, p


def search(D2, perplexity, tol, max_steps, dtype):
    """beta [N] (dtype): scikit-learn's _binary_search_perplexity per row — the LAST EVALUATED beta."""
    n = D2.shape[0]
    target = np.log(perplexity)
    beta = np.ones(n, dtype=dtype)
    lo = np.full(n, -np.inf, dtype=dtype)
    hi = np.full(n, np.inf, dtype=dtype)
    live = np.ones(n, dtype=bool)
    for step in range(max_steps):
        H, _, _ = entropies(D2, beta, dtype)
        diff = H - target
        live &= ~(np.abs(diff) <= tol)
        if step + 1 >= max_steps or not live.any():
            break
        up = live & (diff > 0)
        down = live & ~(diff > 0)
        new = beta.copy()
        lo[up] = beta[up]
        new[up] = np.where(np.isinf(hi[up]), beta[up] * dtype(2), (beta[up] + hi[up]) * dtype(0.5))
        hi[down] = beta[down]
        new[down] = np.where(np.isinf(lo[down]), beta[down] * dtype(0.5), (beta[down] + lo[down]) * dtype(0.5))
        beta = new.astype(dtype)
    return beta


def affinities(X, perplexity, tol=1e-5, max_steps=100, dtype=np.float64):
    """(P [N, N], beta [N], plogp) as sg_tsne_affinities defines them."""
    D2 = distances(X, dtype)
    n = D2.shape[0]
    beta = search(D2, perplexity, tol, max_steps, dtype)
    _, sum_p, p = entropies(D2, beta, dtype)
    cond = (p.astype(np.float64) / sum_p[:, None]).astype(dtype)
    P = ((cond + cond.T) / dtype(2 * n)).astype(dtype)
    return P, beta, plogp(P)


def plogp(P):
    p = P.astype(np.float64)
    p = p[p > 0]
    return float((p * np.log(p)).sum())


def row_entropy_at(X, beta, dtype):
    """The entropy of every row's conditional distribution at the given beta, evaluated in `dtype` (sums in float64)."""
    return entropies(distances(X, dtype), np.asarray(beta), dtype)[0]


def gradient(Y, P, exaggeration, plogp_value, dtype=np.float64, rows=None):
    """(grad [N, 2] float64-summed, kl) as sg_tsne_gradient defines them; rows: the gradient of these rows only (Z and kl still take
    every pair)."""
    Y, P = Y.astype(dtype), P.astype(dtype)
    dx, dy = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]
    q = (dx * dx + dy * dy).astype(dtype)
    w = (dtype(1) / (dtype(1) + q)).astype(dtype)
    np.fill_diagonal(w, 0)
    Z = w.sum(axis=1, dtype=np.float64).sum()
    k = (P * np.log1p(q)).astype(dtype).sum(axis=1, dtype=np.float64)
    sel = slice(None) if rows is None else np.asarray(rows)
    pw, w2 = (P[sel] * w[sel]).astype(dtype), (w[sel] * w[sel]).astype(dtype)
    a = np.stack([(pw * dx[sel]).astype(dtype).sum(axis=1, dtype=np.float64), (pw * dy[sel]).astype(dtype).sum(axis=1, dtype=np.float64)], axis=1)
    r = np.stack([(w2 * dx[sel]).astype(dtype).sum(axis=1, dtype=np.float64), (w2 * dy[sel]).astype(dtype).sum(axis=1, dtype=np.float64)], axis=1)
    grad = 4.0 * (np.float64(dtype(exaggeration)) * a - r / Z)
    return grad.astype(dtype), float(plogp_value + k.sum() + np.log(Z))


def update(Y, velocity, gains, grad, momentum, lr, min_gain=0.01, dtype=np.float64):
    """scikit-learn's _gradient_descent step: new (Y, velocity, gains)."""
    Y, velocity, gains, grad = (t.astype(dtype) for t in (Y, velocity, gains, grad))
    inc = velocity * grad < 0
    gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8)).astype(dtype)
    gains = np.maximum(gains, dtype(min_gain))
    velocity = (dtype(momentum) * velocity - dtype(lr) * (gains * grad)).astype(dtype)
    return (Y + velocity).astype(dtype), velocity, gains


def run(P, Y0, iterations=1000, exaggeration=12.0, exaggeration_iterations=250, lr=None):
    """The whole optimisation in float64 from Y0: (Y, final kl of the un-exaggerated P)."""
    n = len(Y0)
    lr = lr or max(n / exaggeration / 4.0, 50.0)
    Y, U, gains = Y0.astype(np.float64), np.zeros((n, 2)), np.ones((n, 2))
    for it in range(iterations):
        early = it < exaggeration_iterations
        g, _ = gradient(Y, P, exaggeration if early else 1.0, 0.0)
        Y, U, gains = update(Y, U, gains, g, 0.5 if early else 0.8, lr)
    return Y, gradient(Y, P, 1.0, plogp(P))[1]
