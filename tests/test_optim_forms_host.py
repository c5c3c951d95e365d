"""The float64 formulas that tests/optim_forms.py holds the optimizer kernels against walk the trajectory of torch.optim.Adam and
torch.optim.RMSprop in float64 (no GPU, no library): 20 steps, two parameters, one of which skips a step."""
import pytest
import torch

import optim_forms as O

STEPS, SKIP_AT = 20, 7


def _close(a, b, what):
    err = float(((a - b).abs() / b.abs().clamp(min=1e-300)).max())
    assert err <= 1e-12, "%s: %.3g relative" % (what, err)


@pytest.mark.parametrize("lr,b1,b2", O.ADAM_HYPER)
def test_adam_formula_walks_torch_float64(lr, b1, b2):
    torch.manual_seed(11)
    params = [torch.randn(50, dtype=torch.float64).requires_grad_(True), torch.randn(7, dtype=torch.float64).requires_grad_(True)]
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=O.EPS)
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p), 0) for p in params]
    for k in range(STEPS):
        for i, p in enumerate(params):
            if i == 1 and k == SKIP_AT:
                p.grad = None            # skipped: it neither moves nor ages
                continue
            p.grad = torch.randn_like(p) * (10.0 ** (k % 5 - 2))
            q, m, v, t = mine[i]
            r = O.adam_formula(q, p.grad, m, v, lr, b1, b2, O.EPS, t + 1)
            mine[i] = (r["p"], r["m"], r["v"], t + 1)
        opt.step()
        for i, p in enumerate(params):
            _close(mine[i][0], p.detach(), "Adam step %d parameter %d" % (k, i))
            if p in opt.state:
                _close(mine[i][1], opt.state[p]["exp_avg"], "Adam step %d exp_avg %d" % (k, i))
                _close(mine[i][2], opt.state[p]["exp_avg_sq"], "Adam step %d exp_avg_sq %d" % (k, i))
    assert mine[1][3] == STEPS - 1 and mine[0][3] == STEPS


@pytest.mark.parametrize("alpha,clip", [(0.99, 0.0), (0.9, 0.0), (0.99, 0.5)])
def test_rmsprop_formula_walks_torch_float64(alpha, clip):
    torch.manual_seed(12)
    lr = 1e-3
    params = [torch.randn(50, dtype=torch.float64).requires_grad_(True), torch.randn(7, dtype=torch.float64).requires_grad_(True)]
    opt = torch.optim.RMSprop(params, lr=lr, alpha=alpha, eps=O.EPS)
    mine = [(p.detach().clone(), torch.zeros_like(p)) for p in params]
    for k in range(STEPS):
        for i, p in enumerate(params):
            if i == 1 and k == SKIP_AT:
                p.grad = None
                continue
            p.grad = torch.randn_like(p) * (10.0 ** (k % 5 - 2))
            r = O.rms_formula(mine[i][0], p.grad, mine[i][1], lr, alpha, O.EPS, 1.0, clip)
            mine[i] = (r["p"], r["sq"])
        opt.step()
        if clip > 0:
            with torch.no_grad():
                for p in params:
                    p.clamp_(-clip, clip)        # the reference's clip_weights after the step
        for i, p in enumerate(params):
            _close(mine[i][0], p.detach(), "RMSprop step %d parameter %d" % (k, i))
            if p in opt.state:
                _close(mine[i][1], opt.state[p]["square_avg"], "RMSprop step %d square_avg %d" % (k, i))
