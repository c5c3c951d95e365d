"""Inputs, float64 references and test bodies of the latent fit: SDFNet.latent_loss_and_grad (csrc/latent_fit.hip and its twin) and
shapegan_amd/reconstruct.py.  Run on the twin by tests/test_latent_fit.py and on the GPU by tests/test_gpu_latent_fit.py; nothing here is
a test by itself.

Reference.  oracle.torch_oracle.sdfnet_forward on a float64 copy of the state and inputs, and again in float32, with autograd of the
per-shape objective
    mean_p |f(x_p, z_s) - clamp(sdf_p, +-cutoff)| + sigma * mean_k z_{s,k}^2.
Criterion.  sdfnet_forms.check:  |got - ref64| <= 1e-4 * mean|ref64| + 4 * max|ref32 - ref64|, for `loss` and for `grad`.
Kinks.  The upstream gradient is formed inside the kernel, so it cannot be masked from outside: twice the points needed are drawn
and the first ones kept whose float64 min |pre-activation| >= 1e-6 and whose float64 |out - clamp(target)| >= 1e-3 (the kink of the L1
loss).  The fragile share of what is kept is 0; that enough points remained is asserted.  The decision uses the reference alone."""
import functools
import os

import numpy as np
import pytest
import torch

import test_gpu_ops as OPS
from oracle import torch_oracle as O
from sdfnet_forms import check, fragile_points, make_net, segment_table

CUTOFF = 0.1
L1_KINK = 1e-3
POSITION_RUNS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 2]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def net_on(dev, seed, latent, state=None):
    old, OPS.DEV = OPS.DEV, dev
    try:
        net = make_net(seed, latent)
    finally:
        OPS.DEV = old
    if state is not None:
        net.load_state_dict(state)
    return net


def chairs_state():
    z = np.load(os.path.join(GOLDEN, "sdfnet_chairs_weights.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def state_of(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def objective(sd, pts, tgt, z, seg_off, cutoff, sigma, dtype):
    """(loss [S], grad [S, L]) of the per-shape objective in `dtype` by autograd."""
    P = {k: v.to(dtype) for k, v in sd.items()}
    counts = seg_off[1:] - seg_off[:-1]
    sid = torch.repeat_interleave(torch.arange(counts.numel()), counts)
    zz = z.to(dtype).clone().requires_grad_(True)
    out = O.sdfnet_forward(P, pts.to(dtype), zz[sid]).reshape(-1)
    d = (out - tgt.to(dtype).clamp(-cutoff, cutoff)).abs()
    loss = torch.zeros(counts.numel(), dtype=dtype).index_add(0, sid, d) / counts.to(dtype)
    (loss.sum() + sigma * (zz * zz).mean(dim=1).sum()).backward()
    return loss.detach(), zz.grad


def safe_points(sd, z, runs, seed, cutoff=CUTOFF, target=None):
    """(points [N,3], targets [N], seg_off): per shape twice the points drawn, the first safe ones kept (module docstring).
    target: None — N(0, 0.1^2) values, a third of them beyond +-cutoff — or a function (points float64, shape) -> values."""
    g = torch.Generator().manual_seed(seed)
    P64 = {k: v.double() for k, v in sd.items()}
    pts, tgt = [], []
    for s, n in enumerate(runs):
        cand = torch.rand(2 * n + 8, 3, generator=g) * 2 - 1
        t = torch.randn(2 * n + 8, generator=g) * 0.1 if target is None else target(cand.double(), s).float()
        zs = z[s:s + 1].expand(cand.shape[0], -1)
        fragile = fragile_points(sd, cand, zs, None)
        with torch.no_grad():
            out = O.sdfnet_forward(P64, cand.double(), zs.double()).reshape(-1)
        ok = ~fragile & ((out - t.double().clamp(-cutoff, cutoff)).abs() >= L1_KINK)
        keep = ok.nonzero().flatten()[:n]
        assert keep.numel() == n, "shape %d: only %d of %d candidate points are safe, %d needed" % (s, int(ok.sum()), cand.shape[0], n)
        pts.append(cand[keep])
        tgt.append(t[keep])
    return torch.cat(pts), torch.cat(tgt), segment_table(runs)[1]


class Case(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def make_case(weights, latent, runs, seed, sigma):
    """Inputs and both references: made once per (weights, latent, runs, seed, sigma), shared, never written."""
    runs = list(runs)
    sd = chairs_state() if weights == "chairs" else state_of(net_on("cpu", seed, latent))
    z = torch.randn(len(runs), latent, generator=torch.Generator().manual_seed(seed + 1)) * (0.1 if weights == "chairs" else 0.5)
    pts, tgt, seg_off = safe_points(sd, z, runs, seed + 2)
    assert float((tgt.abs() > CUTOFF).float().mean()) > 0.1, "the targets should reach beyond the cutoff"
    l32, g32 = objective(sd, pts, tgt, z, seg_off, CUTOFF, sigma, torch.float32)
    l64, g64 = objective(sd, pts, tgt, z, seg_off, CUTOFF, sigma, torch.float64)
    return Case(sd=sd, seed=seed, latent=latent, runs=runs, z=z, pts=pts, tgt=tgt, seg_off=seg_off, sigma=sigma, l32=l32, g32=g32, l64=l64, g64=g64)


def run(net, dev, pts, tgt, z, seg_off, **kw):
    loss, grad = net.latent_loss_and_grad(pts.to(dev), tgt.to(dev), z.to(dev), seg_off.to(dev), **kw)
    assert loss.device.type == torch.device(dev).type and grad.device.type == torch.device(dev).type
    return loss.cpu(), grad.cpu()


def check_case(body, dev, case, fused=True):
    net = net_on(dev, case.seed, case.latent, case.sd)
    loss, grad = run(net, dev, case.pts, case.tgt, case.z, case.seg_off, cutoff=CUTOFF, sigma=case.sigma, fused=fused)
    check(body, loss, case.l32, case.l64, "loss")
    check(body, grad, case.g32, case.g64, "latent gradient")
    for p in net.parameters():
        assert p.grad is None, "a parameter received a .grad"


# ---- bodies -----------------------------------------------------------------------------------------------------------------------
def body_positions(dev, weights, sigma):
    """Every tile position: runs of 1 .. 200 points (one lane, a full tile less one, full tiles, one more, several tiles) in one call."""
    check_case("positions %s sigma %g" % (weights, sigma), dev, make_case(weights, 128, tuple(POSITION_RUNS), 31, sigma))


def body_latent_sizes(dev, latent):
    check_case("latent size %d" % latent, dev, make_case("seeded", latent, (33, 64, 5), 40 + latent, 0.01))


def body_composed(dev):
    check_case("composed path", dev, make_case("seeded", 128, tuple(POSITION_RUNS), 31, 0.01), fused=False)


def _slice(case, order):
    """The case restricted to the shapes `order`, in that order."""
    so = case.seg_off.tolist()
    idx = torch.cat([torch.arange(so[s], so[s + 1]) for s in order])
    return case.pts[idx], case.tgt[idx], case.z[list(order)], segment_table([case.runs[s] for s in order])[1]


def body_independence(dev):
    """A shape's loss and gradient row do not depend on what else is in the call, or where in the call it stands: bit for bit."""
    case = make_case("seeded", 128, (70, 33, 129), 52, 0.01)
    net = net_on(dev, case.seed, case.latent, case.sd)
    for s in range(3):
        alone = run(net, dev, *_slice(case, [s]), cutoff=CUTOFF, sigma=0.01)
        others = [t for t in range(3) if t != s]
        for pos in range(3):
            order = others[:pos] + [s] + others[pos:]
            loss, grad = run(net, dev, *_slice(case, order), cutoff=CUTOFF, sigma=0.01)
            assert torch.equal(loss[pos], alone[0][0]), "shape %d at position %d: loss %r, alone %r" % (s, pos, float(loss[pos]), float(alone[0][0]))
            assert torch.equal(grad[pos], alone[1][0]), "shape %d at position %d: the gradient row differs from the shape alone" % (s, pos)


WINDOWS = [(0, 0), (0, 40), (50, 64), (190, 64), (7, 1000)]


def body_windows(dev, window):
    """A window equals a call on the explicitly gathered points, bit for bit ((190, 64) wraps; (7, 1000) is every point, rotated)."""
    case = make_case("seeded", 128, (200, 77), 61, 0.0)
    net = net_on(dev, case.seed, case.latent, case.sd)
    start, count = window
    so = case.seg_off.tolist()
    idx, runs = [], []
    for s in range(2):
        n = so[s + 1] - so[s]
        m = n if count <= 0 else min(count, n)
        idx.append(so[s] + (start + torch.arange(m)) % n)
        runs.append(m)
    idx = torch.cat(idx)
    got = run(net, dev, case.pts, case.tgt, case.z, case.seg_off, cutoff=CUTOFF, sigma=0.01, window=window)
    exp = run(net, dev, case.pts[idx], case.tgt[idx], case.z, segment_table(runs)[1], cutoff=CUTOFF, sigma=0.01)
    assert torch.equal(got[0], exp[0]), "window %s: loss %s, gathered %s" % (window, got[0], exp[0])
    assert torch.equal(got[1], exp[1]), "window %s: the gradient differs from the gathered call" % (window,)
    if window == (0, 0):
        check("windows", got[0], case.l32, case.l64, "loss")


def body_exact_zero(dev):
    """Targets = the forward's own output: d == 0 at every point, so loss and gradient are exact zeros — only if the fused forward
    is the existing one bit for bit and sign(0) = 0."""
    case = make_case("seeded", 128, (70, 33, 129), 52, 0.01)
    net = net_on(dev, case.seed, case.latent, case.sd)
    sid, seg_off = segment_table(case.runs)
    with torch.no_grad():
        out = net.forward_segments(case.pts.to(dev), case.z.to(dev), sid.int().to(dev), seg_off.to(dev)).cpu()
    assert float(out.abs().max()) < 1.0
    loss, grad = run(net, dev, case.pts, out, case.z, case.seg_off, cutoff=1.0, sigma=0.0)
    assert torch.equal(loss, torch.zeros_like(loss)), "loss %s" % loss
    assert torch.equal(grad, torch.zeros_like(grad)), "largest gradient entry %g" % float(grad.abs().max())


def body_chunking(dev, monkeypatch):
    """More shapes than one call of the fold's backward takes go in chunks: with the limit at 3, seven shapes equal the unchunked call."""
    from shapegan_amd import ops
    case = make_case("seeded", 30, (33, 5, 64, 1, 40, 65, 2), 70, 0.01)
    net = net_on(dev, case.seed, case.latent, case.sd)
    whole = run(net, dev, case.pts, case.tgt, case.z, case.seg_off, cutoff=CUTOFF, sigma=0.01, window=(3, 48))
    monkeypatch.setattr(ops, "_LATENT_MAX_SHAPES", 3)
    parts = run(net, dev, case.pts, case.tgt, case.z, case.seg_off, cutoff=CUTOFF, sigma=0.01, window=(3, 48))
    assert torch.equal(parts[0], whole[0]) and torch.equal(parts[1], whole[1])


def body_refusals(dev, monkeypatch):
    """Bad arguments raise before anything is launched."""
    from shapegan_amd import ops
    case = make_case("seeded", 30, (33, 5, 64, 1, 40, 65, 2), 70, 0.01)
    net = net_on(dev, case.seed, case.latent, case.sd)

    def no_library():
        raise AssertionError("a library call was assembled for a refused argument")
    monkeypatch.setattr(ops, "_lib", no_library)
    pts, tgt, z, so = case.pts.to(dev), case.tgt.to(dev), case.z.to(dev), case.seg_off.to(dev)
    empty = so.clone()
    empty[3] = empty[2]
    for fused in (True, False):
        with pytest.raises(ValueError, match="no points"):
            net.latent_loss_and_grad(pts, tgt, z, empty, fused=fused)
        with pytest.raises(ValueError, match="rows"):
            net.latent_loss_and_grad(pts, tgt, z[:-1], so, fused=fused)
        with pytest.raises(ValueError, match=r"\[N, 3\]"):
            net.latent_loss_and_grad(pts[:, :2], tgt, z, so, fused=fused)
        with pytest.raises(ValueError, match="window"):
            net.latent_loss_and_grad(pts, tgt, z, so, window=(-1, 4), fused=fused)


# ---- the fit ----------------------------------------------------------------------------------------------------------------------
FIT_RUNS = (96, 64, 33, 130)
FIT_ITERS, FIT_LR, FIT_SIGMA = 10, 1e-3, 0.01


def adam_reference(sd, pts, tgt, seg_off, latent, dtype):
    """(codes after FIT_ITERS torch.optim.Adam steps from zero, data term before, data term after) in `dtype`."""
    P = {k: v.to(dtype) for k, v in sd.items()}
    counts = seg_off[1:] - seg_off[:-1]
    sid = torch.repeat_interleave(torch.arange(counts.numel()), counts)
    z = torch.zeros(counts.numel(), latent, dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([z], lr=FIT_LR)
    p, t = pts.to(dtype), tgt.to(dtype).clamp(-CUTOFF, CUTOFF)

    def data_term():
        d = (O.sdfnet_forward(P, p, z[sid]).reshape(-1) - t).abs()
        return torch.zeros(counts.numel(), dtype=dtype).index_add(0, sid, d) / counts.to(dtype)
    first = data_term().detach()
    for _ in range(FIT_ITERS):
        opt.zero_grad()
        (data_term().sum() + FIT_SIGMA * (z * z).mean(dim=1).sum()).backward()
        opt.step()
    return z.detach(), first, data_term().detach()


@functools.lru_cache(maxsize=None)
def fit_case():
    latent, seed = 64, 81
    sd = state_of(net_on("cpu", seed, latent))
    hidden = torch.randn(len(FIT_RUNS), latent, generator=torch.Generator().manual_seed(seed + 1)) * 0.5
    P64 = {k: v.double() for k, v in sd.items()}

    def target(points, s):      # the hidden code through the float64 net
        with torch.no_grad():
            return O.sdfnet_forward(P64, points, hidden[s:s + 1].double().expand(points.shape[0], -1)).reshape(-1)
    pts, tgt, seg_off = safe_points(sd, torch.zeros_like(hidden), list(FIT_RUNS), seed + 2, target=target)
    z32, _, last32 = adam_reference(sd, pts, tgt, seg_off, latent, torch.float32)
    z64, first, last = adam_reference(sd, pts, tgt, seg_off, latent, torch.float64)
    assert bool((last < first).all()), "the float64 fit should lower every shape's loss: %s -> %s" % (first, last)
    return Case(sd=sd, seed=seed, latent=latent, pts=pts, tgt=tgt, seg_off=seg_off, z32=z32, z64=z64, last=last, last32=last32)


def body_fit(dev, fused=True):
    from shapegan_amd.reconstruct import fit_latent_codes
    case = fit_case()
    net = net_on(dev, case.seed, case.latent, case.sd)
    before = [p.detach().clone() for p in net.parameters()]
    kw = dict(iterations=FIT_ITERS, lr=FIT_LR, sigma=FIT_SIGMA, cutoff=CUTOFF, fused=fused)
    codes, loss = fit_latent_codes(net, case.pts.to(dev), case.tgt.to(dev), case.seg_off.to(dev), **kw)
    body = "fit" if fused else "fit composed"
    check(body, codes, case.z32, case.z64, "codes after %d Adam steps" % FIT_ITERS)
    check(body, loss, case.last32, case.last, "returned loss")
    for p, q in zip(net.parameters(), before):
        assert torch.equal(p.detach(), q) and p.grad is None, "the fit touched a parameter"
    if fused:
        so = case.seg_off.tolist()
        for s in (0, 3):
            sl = slice(so[s], so[s + 1])
            alone, l1 = fit_latent_codes(net, case.pts[sl].to(dev), case.tgt[sl].to(dev), points_per_shape=so[s + 1] - so[s], **kw)
            assert torch.equal(alone[0].cpu(), codes[s].cpu()), "shape %d fitted alone differs from its row in the batch" % s
            assert torch.equal(l1[0].cpu(), loss[s].cpu())


def body_fit_windows(dev):
    """Mini-batch windows through shuffled clouds: the loop runs, is repeatable bit for bit, and lowers the loss it reports."""
    from shapegan_amd.reconstruct import fit_latent_codes
    case = fit_case()
    net = net_on(dev, case.seed, case.latent, case.sd)
    kw = dict(iterations=6, lr=FIT_LR, points_per_step=48, seed=3)
    a = fit_latent_codes(net, case.pts.to(dev), case.tgt.to(dev), case.seg_off.to(dev), **kw)
    b = fit_latent_codes(net, case.pts.to(dev), case.tgt.to(dev), case.seg_off.to(dev), **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    zero = net.latent_loss_and_grad(case.pts.to(dev), case.tgt.to(dev), torch.zeros_like(a[0]), case.seg_off.to(dev))[0]
    assert bool((a[1] < zero).all()), "loss %s after the fit, %s at the start" % (a[1], zero)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def body_meshes(dev):
    """Two fitted codes through reconstruct_meshes at resolution 16: each shape is get_mesh of its code, bit for bit."""
    from shapegan_amd.reconstruct import fit_latent_codes, reconstruct_meshes
    sd = chairs_state()
    latent = sd["layers1.0.weight"].shape[1] - 3
    net = net_on(dev, 5, latent, sd)
    g = torch.Generator().manual_seed(9)
    pts = torch.rand(2, 150, 3, generator=g) * 2 - 1
    sdf = torch.stack([pts[0].norm(dim=1) - 0.5, pts[1].abs().max(dim=1).values - 0.4])
    codes, _ = fit_latent_codes(net, pts.to(dev), sdf.to(dev), iterations=3, lr=5e-3)
    batch = reconstruct_meshes(net, codes, voxel_resolution=16)
    assert len(batch) == 2 and int(batch.faces.shape[0]) > 0, "the chairs network should give a surface at resolution 16"
    for s in range(2):
        one = net.get_mesh(codes[s], voxel_resolution=16)
        got = batch.mesh(s)
        if one is None:
            assert got.faces.shape[0] == 0
            continue
        assert np.array_equal(got.vertices, one.vertices) and np.array_equal(got.faces, one.faces)
        assert np.array_equal(got.vertex_normals, one.vertex_normals)


TETRAHEDRA = """v 0 0 0
v 1 0 0
v 0 1 0
v 0 0 1
f 1 3 2
f 1 2 4
f 1 4 3
f 2 3 4
v 2 2 2
v 3 2 2
v 2 3 2
v 2 2 3
f 5 7 6
f 5 6 8
f 5 8 7
f 6 7 8
"""


def body_cli(tmp_path, capsys):
    """The command line on a two-tetrahedron .obj, on the CPU: codes saved, one mesh file, a Chamfer line."""
    from shapegan_amd import reconstruct
    models = tmp_path / "models" / "abc" / "models"
    models.mkdir(parents=True)
    (models / "model_normalized.obj").write_text(TETRAHEDRA)
    torch.save(chairs_state(), str(tmp_path / "sdf_net.to"))
    out = tmp_path / "out" / "codes.to"
    rc = reconstruct.main(["--net", str(tmp_path / "sdf_net.to"), "--models", str(tmp_path / "models"), "--out", str(out), "--meshes",
                           str(tmp_path / "meshes"), "--chamfer", "--device", "cpu", "--points", "300", "--iterations", "2",
                           "--scan-count", "6", "--scan-resolution", "64", "--resolution", "16", "--chamfer-points", "64"])
    assert rc == 0
    codes = torch.load(str(out))
    assert codes.shape == (1, 128) and codes.dtype == torch.float32 and bool(torch.isfinite(codes).all()) and float(codes.abs().max()) > 0
    assert (tmp_path / "meshes" / "0000.obj").exists()
    text = capsys.readouterr().out
    assert "model_normalized.obj: loss" in text and "chamfer" in text
