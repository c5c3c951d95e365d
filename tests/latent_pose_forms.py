"""Inputs, float64 references and test bodies of the pose fit: SDFNet.latent_pose_loss_and_grad (csrc/latent_fit.hip and its twin),
ops.LatentPoseFit and reconstruct.fit_codes_and_poses.  Run on the twin by tests/test_latent_pose.py and on the GPU by
tests/test_gpu_latent_pose.py; nothing here is a test by itself.

Reference.  oracle.torch_oracle.sdfnet_forward on a float64 copy of the state and inputs, and again in float32, with autograd of the
per-shape objective
    mean_p |f(A_s q_p + t_s, z_s) - clamp(ts_s sdf_p, +-cutoff)| + sigma * mean_k z_{s,k}^2
with respect to the code, A|t and ts.
Criterion.  sdfnet_forms.check:  |got - ref64| <= 1e-4 * mean|ref64| + 4 * max|ref32 - ref64|, for `loss`, `grad_z` and the 13 live
floats of `grad_pose`.
Kinks.  Twice the points needed are drawn and the first ones kept whose float64 min |pre-activation| >= 1e-6 (at the POSED point),
whose |out - target'| >= 1e-3 (the kink of the L1 loss) and whose ||ts target| - cutoff| >= 1e-3 (the kink of the clamp, which the
gradient with respect to ts sees).  That at most half of the candidates are dropped is asserted; the decision uses the float64
reference alone."""
import functools
import math
import re

import pytest
import torch

from latent_fit_forms import CUTOFF, L1_KINK, Case, chairs_state, net_on
from oracle import torch_oracle as O
from project_forms import weights_of
from sdfnet_forms import check, fragile_points, segment_table

CLAMP_KINK = 1e-3
SG_ERR_ARG = -1      # csrc/common.h
RUNS = (1, 31, 32, 33, 64, 65, 200)
POSES = ("identity", "similarity", "affine")


def seeded_state(seed, latent):
    """A seeded state with every hidden layer's weight times sqrt(6) and a surface in the cube: tests/project_forms.py's."""
    return weights_of("seeded", seed, latent)


def rodrigues(axis, angle):
    """The written-out formula, float64: R = I + sin(a) K + (1 - cos(a)) K^2 for a unit axis."""
    a = torch.as_tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def pose_rows_of(kind, S, seed):
    """[S,16] float32 pose rows: the identity, a generic similarity (20 degrees, |t| = 0.1, s = 1.2) or a generic non-orthogonal
    affine with ts != 1; floats 13..15 hold junk the kernel must ignore."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.zeros(S, 16, dtype=torch.float64)
    for s in range(S):
        if kind == "identity":
            A, t, ts = torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), 1.0
        elif kind == "similarity":
            axis = torch.randn(3, generator=g, dtype=torch.float64)
            t = torch.randn(3, generator=g, dtype=torch.float64)
            A, t, ts = 1.2 * rodrigues(axis, math.radians(20)), 0.1 * t / t.norm(), 1.2
        else:
            A = torch.eye(3, dtype=torch.float64) + 0.25 * (torch.rand(3, 3, generator=g, dtype=torch.float64) * 2 - 1)
            t = 0.1 * (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1)
            ts = 0.8 + 0.1 * s
        rows[s, :12] = torch.cat([A, t[:, None]], dim=1).reshape(12)
        rows[s, 12] = ts
        rows[s, 13:] = torch.tensor([7.0, -3.0, 1e30], dtype=torch.float64)
    return rows.float()


def posed(pose, sid, pts):
    """x = A q + t and ts per point, in the dtype of `pose`."""
    M = pose[:, :12].reshape(-1, 3, 4)[sid]
    return (M[:, :, :3] * pts[:, None, :]).sum(dim=2) + M[:, :, 3], pose[:, 12][sid]


def objective(sd, pts, tgt, z, pose, seg_off, cutoff, sigma, dtype):
    """(loss [S], grad_z [S,L], grad_pose [S,16]) of the per-shape objective in `dtype` by autograd."""
    P = {k: v.to(dtype) for k, v in sd.items()}
    counts = seg_off[1:] - seg_off[:-1]
    sid = torch.repeat_interleave(torch.arange(counts.numel()), counts)
    zz = z.to(dtype).clone().requires_grad_(True)
    pp = pose.to(dtype).clone().requires_grad_(True)
    x, ts = posed(pp, sid, pts.to(dtype))
    out = O.sdfnet_forward(P, x, zz[sid]).reshape(-1)
    d = (out - (ts * tgt.to(dtype)).clamp(-cutoff, cutoff)).abs()
    loss = torch.zeros(counts.numel(), dtype=dtype).index_add(0, sid, d) / counts.to(dtype)
    (loss.sum() + sigma * (zz * zz).mean(dim=1).sum()).backward()
    gp = pp.grad.clone()
    gp[:, 13:] = 0
    return loss.detach(), zz.grad, gp


def safe_points(sd, z, pose, runs, seed, cutoff=CUTOFF, target=None):
    """(points [N,3], targets [N], seg_off): per shape twice the points drawn, the first safe ones kept (module docstring).
    target: None — N(0, 0.1^2) values, a good share of them beyond +-cutoff after the scale — or a function (posed points float64,
    shape) -> values."""
    g = torch.Generator().manual_seed(seed)
    P64 = {k: v.double() for k, v in sd.items()}
    pts, tgt = [], []
    for s, n in enumerate(runs):
        cand = torch.rand(2 * n + 8, 3, generator=g) * 2 - 1
        x, ts = posed(pose.double(), torch.full((cand.shape[0],), s, dtype=torch.int64), cand.double())
        t = torch.randn(2 * n + 8, generator=g) * 0.1 if target is None else target(x, s).float()
        zs = z[s:s + 1].expand(cand.shape[0], -1)
        fragile = fragile_points(sd, x, zs, None)
        with torch.no_grad():
            out = O.sdfnet_forward(P64, x, zs.double()).reshape(-1)
        st = ts * t.double()
        ok = ~fragile & ((out - st.clamp(-cutoff, cutoff)).abs() >= L1_KINK) & ((st.abs() - cutoff).abs() >= CLAMP_KINK)
        assert int((~ok).sum()) * 2 <= cand.shape[0], "shape %d: %d of %d candidates dropped, more than half" % (s, int((~ok).sum()), cand.shape[0])
        keep = ok.nonzero().flatten()[:n]
        assert keep.numel() == n, "shape %d: only %d of %d candidate points are safe, %d needed" % (s, int(ok.sum()), cand.shape[0], n)
        pts.append(cand[keep])
        tgt.append(t[keep])
    return torch.cat(pts), torch.cat(tgt), segment_table(list(runs))[1]


@functools.lru_cache(maxsize=None)
def make_case(weights, latent, runs, seed, sigma, kind):
    """Inputs and both references: made once per key, shared, never written."""
    runs = list(runs)
    sd = chairs_state() if weights == "chairs" else seeded_state(seed, latent)
    z = torch.randn(len(runs), latent, generator=torch.Generator().manual_seed(seed + 1)) * 0.1
    pose = pose_rows_of(kind, len(runs), seed + 3)
    pts, tgt, seg_off = safe_points(sd, z, pose, runs, seed + 2)
    sid = segment_table(runs)[0]
    st = (pose[:, 12][sid] * tgt).abs()
    assert float((st > CUTOFF).float().mean()) > 0.1 and float((st < CUTOFF).float().mean()) > 0.1, "targets on both sides of the clamp"
    r32 = objective(sd, pts, tgt, z, pose, seg_off, CUTOFF, sigma, torch.float32)
    r64 = objective(sd, pts, tgt, z, pose, seg_off, CUTOFF, sigma, torch.float64)
    return Case(sd=sd, seed=seed, latent=latent, runs=runs, z=z, pose=pose, pts=pts, tgt=tgt, seg_off=seg_off, sigma=sigma, r32=r32, r64=r64)


def run(net, dev, pts, tgt, z, pose, seg_off, **kw):
    out = net.latent_pose_loss_and_grad(pts.to(dev), tgt.to(dev), z.to(dev), pose.to(dev), seg_off.to(dev), **kw)
    assert all(o.device.type == torch.device(dev).type for o in out)
    return tuple(o.cpu() for o in out)


def check_case(body, dev, case):
    net = net_on(dev, case.seed, case.latent, case.sd)
    loss, gz, gp = run(net, dev, case.pts, case.tgt, case.z, case.pose, case.seg_off, cutoff=CUTOFF, sigma=case.sigma)
    check(body, loss, case.r32[0], case.r64[0], "loss")
    check(body, gz, case.r32[1], case.r64[1], "latent gradient")
    check(body, gp[:, :12], case.r32[2][:, :12], case.r64[2][:, :12], "gradient of A|t")
    check(body, gp[:, 12], case.r32[2][:, 12], case.r64[2][:, 12], "gradient of ts")
    assert torch.equal(gp[:, 13:], torch.zeros(len(case.runs), 3)), "floats 13..15 of grad_pose"
    if any(k in body for k in ("similarity", "affine")):
        assert float(case.r64[2][:, 12].abs().min()) > 0, "every shape should have targets inside the clamp"
    for p in net.parameters():
        assert p.grad is None, "a parameter received a .grad"


# ---- parity -----------------------------------------------------------------------------------------------------------------------
def body_positions(dev, weights, sigma, kind):
    """Every tile position (one lane, a tile less one, a full tile, one more, two tiles, one more, seven tiles less 24) in one call:
    seven shapes, one per run length."""
    check_case("pose positions %s sigma %g %s" % (weights, sigma, kind), dev, make_case(weights, 128, RUNS, 131, sigma, kind))


def body_latent_sizes(dev, latent, sigma):
    check_case("pose latent size %d sigma %g affine" % (latent, sigma), dev, make_case("seeded", latent, (33, 64, 5), 140 + latent, sigma, "affine"))


# ---- bit identities ---------------------------------------------------------------------------------------------------------------
def _fit_objects(dev, case, window=(0, 0)):
    """(LatentFit, LatentPoseFit) of the case on `dev`, and its tensors there."""
    from shapegan_amd import ops
    net = net_on(dev, case.seed, case.latent, case.sd)
    pts, tgt, so = case.pts.to(dev), case.tgt.to(dev), case.seg_off.to(dev)
    off = ops.check_segments(pts, tgt, case.z.to(dev), so)
    args = (net._pack_shapes, net._params(), pts, tgt, so, off, CUTOFF)
    return net, ops.LatentFit(*args), ops.LatentPoseFit(*args)


def body_identity_bits(dev, window):
    """Identity pose, ts = 1: loss and grad_z are LatentFit.step's bit for bit, and so are floats [0, 513) of every partial row."""
    import shapegan_amd.lib as LIB
    from shapegan_amd import ops
    case = make_case("seeded", 29, (1, 31, 33, 65, 200), 150, 0.01, "identity")
    net, plain, withpose = _fit_objects(dev, case)
    z, pose = case.z.to(dev), case.pose.to(dev)
    a = plain.step(z, window[0], window[1], 0.01)
    b = withpose.step(z, pose, window[0], window[1], 0.01)
    assert torch.equal(a[0], b[0]), "loss differs from LatentFit.step"
    assert torch.equal(a[1], b[1]), "grad_z differs from LatentFit.step"
    # the raw entry points, row by row
    lib = ops._lib()
    _, _, tiles, tile_off, ntiles = plain._plan(int(window[1]))[0]
    S = len(case.runs)
    w1, b1, w5, b5 = plain.params[0], plain.params[1], plain.params[8], plain.params[9]
    zb1, zb5 = torch.zeros(S, 256, device=dev), torch.zeros(S, 256, device=dev)
    ops.check(lib.sg_sdfnet_shape_bias(ops.ptr(z), S, case.latent, ops.ptr(w1), ops.ptr(b1), ops.ptr(w5), ops.ptr(b5), ops.ptr(zb1),
                                       ops.ptr(zb5), ops.stream()), "shape_bias")
    r0, r1 = LIB.abi.DEFINES["SG_SDFNET_LATENT_PARTIAL_ROW"], LIB.abi.DEFINES["SG_SDFNET_POSE_PARTIAL_ROW"]
    assert (r0, r1) == (513, 528)
    p0 = torch.full((ntiles, r0), float("nan"), device=dev)
    p1 = torch.full((ntiles, r1), float("nan"), device=dev)
    ops.check(lib.sg_sdfnet_latent_grad(ops.ptr(plain.points), ops.ptr(plain.sdf), ops.ptr(plain.seg_off), S, ops.ptr(zb1), ops.ptr(zb5),
                                        ops.ptr(plain.packed), CUTOFF, window[0], window[1], ops.ptr(tiles), ntiles, ops.ptr(p0),
                                        ops.stream()), "latent_grad")
    ops.check(lib.sg_sdfnet_latent_pose_grad(ops.ptr(plain.points), ops.ptr(plain.sdf), ops.ptr(plain.seg_off), S, ops.ptr(zb1),
                                             ops.ptr(zb5), ops.ptr(plain.packed), ops.ptr(pose), CUTOFF, window[0], window[1],
                                             ops.ptr(tiles), ntiles, ops.ptr(p1), ops.stream()), "latent_pose_grad")
    assert not torch.isnan(p1).any(), "an element of a partial row was not written"
    assert torch.equal(p0, p1[:, :513]), "floats [0, 513) of the partial rows differ from sg_sdfnet_latent_grad's"
    assert torch.equal(p1[:, 526:], torch.zeros(ntiles, 2, device=dev))


def _slice(case, order):
    so = case.seg_off.tolist()
    idx = torch.cat([torch.arange(so[s], so[s + 1]) for s in order])
    return case.pts[idx], case.tgt[idx], case.z[list(order)], case.pose[list(order)], segment_table([case.runs[s] for s in order])[1]


def _same(a, b, what):
    for x, y, name in zip(a, b, ("loss", "grad_z", "grad_pose")):
        assert torch.equal(x, y), "%s: %s differs" % (what, name)


def body_independence(dev):
    """A shape's outputs do not depend on what else is in the call, or where it stands; a repeat is identical."""
    case = make_case("seeded", 29, (70, 33, 129), 152, 0.01, "affine")
    net = net_on(dev, case.seed, case.latent, case.sd)
    kw = dict(cutoff=CUTOFF, sigma=0.01)
    whole = run(net, dev, case.pts, case.tgt, case.z, case.pose, case.seg_off, **kw)
    _same(whole, run(net, dev, case.pts, case.tgt, case.z, case.pose, case.seg_off, **kw), "repeat")
    for s in range(3):
        alone = run(net, dev, *_slice(case, [s]), **kw)
        others = [t for t in range(3) if t != s]
        for pos in range(3):
            order = others[:pos] + [s] + others[pos:]
            got = run(net, dev, *_slice(case, order), **kw)
            _same([g[pos] for g in got], [a[0] for a in alone], "shape %d at position %d against the shape alone" % (s, pos))


WINDOWS = [(0, 40), (190, 64), (7, 1000)]


def body_windows(dev, window):
    """A window equals a call on the explicitly gathered points, bit for bit ((190, 64) wraps; (7, 1000) is every point, rotated)."""
    case = make_case("seeded", 29, (200, 77), 161, 0.0, "similarity")
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
    got = run(net, dev, case.pts, case.tgt, case.z, case.pose, case.seg_off, cutoff=CUTOFF, sigma=0.01, window=window)
    exp = run(net, dev, case.pts[idx], case.tgt[idx], case.z, case.pose, segment_table(runs)[1], cutoff=CUTOFF, sigma=0.01)
    _same(got, exp, "window %s against the gathered call" % (window,))


def body_chunking(dev, monkeypatch):
    """Chunks of two shapes equal the unchunked call."""
    from shapegan_amd import ops
    case = make_case("seeded", 29, (33, 5, 64, 1, 40), 170, 0.01, "affine")
    net = net_on(dev, case.seed, case.latent, case.sd)
    kw = dict(cutoff=CUTOFF, sigma=0.01, window=(3, 48))
    whole = run(net, dev, case.pts, case.tgt, case.z, case.pose, case.seg_off, **kw)
    monkeypatch.setattr(ops, "_LATENT_MAX_SHAPES", 2)
    _same(run(net, dev, case.pts, case.tgt, case.z, case.pose, case.seg_off, **kw), whole, "chunks of two shapes")


def body_exact_zero(dev):
    """Targets = the forward's own output at the posed points: loss, grad_z (sigma = 0) and grad_pose are exact zeros."""
    case = make_case("seeded", 29, (70, 33, 129), 152, 0.01, "affine")
    net = net_on(dev, case.seed, case.latent, case.sd)
    pose = case.pose.clone()
    pose[:, 12] = 1.0
    sid, seg_off = segment_table(case.runs)
    # x as the header forms it: three nested float32 fmas, here in float64 products of float32 values rounded once per fma
    M = pose[:, :12].reshape(-1, 3, 4)[sid].double()
    q = case.pts.double()
    x = M[:, :, 3]
    for j in (2, 1, 0):
        x = (M[:, :, j] * q[:, j:j + 1] + x).float().double()
    x = x.float()
    with torch.no_grad():
        out = net.forward_segments(x.to(dev), case.z.to(dev), sid.int().to(dev), seg_off.to(dev)).cpu()
    assert float(out.abs().max()) < 1.0
    loss, gz, gp = run(net, dev, case.pts, out, case.z, pose, case.seg_off, cutoff=1.0, sigma=0.0)
    assert torch.equal(loss, torch.zeros_like(loss)), "loss %s" % loss
    assert torch.equal(gz, torch.zeros_like(gz)), "largest latent gradient entry %g" % float(gz.abs().max())
    assert torch.equal(gp, torch.zeros_like(gp)), "largest pose gradient entry %g" % float(gp.abs().max())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def body_entry_refusals(dev):
    """Each argument check of the two entry points: SG_ERR_ARG, outputs untouched."""
    from shapegan_amd import ops
    case = make_case("seeded", 29, (33, 5), 180, 0.01, "affine")
    net, plain, _ = _fit_objects(dev, case)
    lib = ops._lib()
    S = 2
    _, _, tiles, tile_off, ntiles = plain._plan(0)[0]
    zb = torch.zeros(S, 256, device=dev)
    pose = case.pose.to(dev)
    part = torch.full((ntiles, 528), 5.0, device=dev)
    good = dict(points=plain.points, target=plain.sdf, seg_off=plain.seg_off, nshapes=S, zb1=zb, zb5=zb, packed=plain.packed, pose=pose,
                cutoff=CUTOFF, win_start=0, win_count=0, tiles=tiles, ntiles=ntiles, partials=part)
    order = ["points", "target", "seg_off", "nshapes", "zb1", "zb5", "packed", "pose", "cutoff", "win_start", "win_count", "tiles", "ntiles", "partials"]

    def call(fn, names, kw):
        return fn(*[ops.ptr(kw[k]) if (kw[k] is None or torch.is_tensor(kw[k])) else kw[k] for k in names], ops.stream())
    bad = [(k, None) for k in order if torch.is_tensor(good[k])] + [("nshapes", 0), ("ntiles", 0), ("ntiles", 1 << 31), ("win_start", -1), ("cutoff", -0.5)]
    for k, v in bad:
        rc = call(lib.sg_sdfnet_latent_pose_grad, order, dict(good, **{k: v}))
        assert rc == SG_ERR_ARG, "latent_pose_grad accepted %s = %r (rc %d)" % (k, v, rc)
    assert torch.equal(part, torch.full_like(part, 5.0)), "a refused call wrote to partials"
    outs = dict(t1=torch.full((256, S), 5.0, device=dev), t5=torch.full((256, S), 5.0, device=dev), loss=torch.full((S,), 5.0, device=dev),
                gpose=torch.full((S, 16), 5.0, device=dev))
    good2 = dict(partials=part, tile_off=tile_off, seg_off=plain.seg_off, nshapes=S, win_count=0, **outs)
    order2 = ["partials", "tile_off", "seg_off", "nshapes", "win_count", "t1", "t5", "loss", "gpose"]
    for k, v in [(k, None) for k in order2 if torch.is_tensor(good2[k])] + [("nshapes", 0)]:
        rc = call(lib.sg_sdfnet_latent_pose_reduce, order2, dict(good2, **{k: v}))
        assert rc == SG_ERR_ARG, "latent_pose_reduce accepted %s = %r (rc %d)" % (k, v, rc)
    for k, t in outs.items():
        assert torch.equal(t, torch.full_like(t, 5.0)), "a refused call wrote to %s" % k


def body_python_refusals(dev, monkeypatch):
    """Each ValueError of the Python layer is raised before anything is launched."""
    from shapegan_amd import ops
    from shapegan_amd.reconstruct import fit_codes_and_poses
    case = make_case("seeded", 29, (33, 5), 180, 0.01, "affine")
    net = net_on(dev, case.seed, case.latent, case.sd)

    def no_library():
        raise AssertionError("a library call was assembled for a refused argument")
    monkeypatch.setattr(ops, "_lib", no_library)
    pts, tgt, z, pose, so = case.pts.to(dev), case.tgt.to(dev), case.z.to(dev), case.pose.to(dev), case.seg_off.to(dev)
    with pytest.raises(ValueError, match=r"\[S, 16\]"):
        net.latent_pose_loss_and_grad(pts, tgt, z, pose[:, :12], so)
    with pytest.raises(ValueError, match=r"\[S, 16\]"):
        net.latent_pose_loss_and_grad(pts, tgt, z, pose[:1], so)
    with pytest.raises(ValueError, match="floating-point"):
        net.latent_pose_loss_and_grad(pts, tgt, z, pose.long(), so)
    if torch.device(dev).type != "cpu":
        with pytest.raises(ValueError, match="pose is on"):
            net.latent_pose_loss_and_grad(pts, tgt, z, pose.cpu(), so)
    with pytest.raises(ValueError, match="window"):
        net.latent_pose_loss_and_grad(pts, tgt, z, pose, so, window=(-1, 4))
    with pytest.raises(ValueError, match="rows"):
        net.latent_pose_loss_and_grad(pts, tgt, z[:-1], pose[:-1], so)
    with pytest.raises(ValueError, match="pose must be one of"):
        fit_codes_and_poses(net, pts, tgt, so, pose="affine")
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="rotation_starts"):
            fit_codes_and_poses(net, pts, tgt, so, rotation_starts=bad)


# ---- the pose map -------------------------------------------------------------------------------------------------------------------
def body_pose_map():
    """theta -> [S,16] and its backward against float64 autograd of the written-out Rodrigues formula; omega = 0 included, where the
    formula's derivative is that of I + K(omega)."""
    from shapegan_amd.reconstruct import pose_rows
    g = torch.Generator().manual_seed(5)
    theta = torch.randn(6, 7, generator=g, dtype=torch.float64) * torch.tensor([0.8] * 3 + [0.3] * 3 + [0.2], dtype=torch.float64)
    theta[0, :3] = 0
    theta[1, :3] = theta[1, :3] / theta[1, :3].norm() * 1e-4      # on the series
    theta[2, :3] = theta[2, :3] / theta[2, :3].norm() * 3.0       # near pi
    up = torch.randn(6, 16, generator=g, dtype=torch.float64)

    def written_out(th):
        rows = []
        for s in range(th.shape[0]):
            w = th[s, :3]
            K = torch.stack([torch.zeros((), dtype=th.dtype), -w[2], w[1], w[2], torch.zeros((), dtype=th.dtype), -w[0], -w[1], w[0],
                             torch.zeros((), dtype=th.dtype)]).reshape(3, 3)
            a = w.norm()
            if float(a.detach()) == 0.0:
                R = torch.eye(3, dtype=th.dtype) + K
            else:
                R = torch.eye(3, dtype=th.dtype) + torch.sin(a) / a * K + (1 - torch.cos(a)) / (a * a) * (K @ K)
            sc = th[s, 6].exp()
            rows.append(torch.cat([torch.cat([sc * R, th[s, 3:6, None]], dim=1).reshape(12), sc[None], torch.zeros(3, dtype=th.dtype)]))
        return torch.stack(rows)
    a = theta.clone().requires_grad_(True)
    ref = written_out(a)
    gref, = torch.autograd.grad(ref, a, up)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2e-6)):
        b = theta.to(dtype).clone().requires_grad_(True)
        rows = pose_rows(b)
        grad, = torch.autograd.grad(rows, b, up.to(dtype))
        assert rows.shape == (6, 16) and rows.dtype == dtype
        assert float((rows.detach().double() - ref.detach()).abs().max()) <= tol * 4, "pose rows, %s" % dtype
        assert float((grad.double() - gref).abs().max()) <= tol * 40, "backward of the pose map, %s: %g" % (dtype, float((grad.double() - gref).abs().max()))
    assert torch.equal(pose_rows(torch.zeros(2, 7))[:, :13], torch.tensor([[1., 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1]] * 2)), "theta = 0 is the identity, exactly"


# ---- ten Adam steps -----------------------------------------------------------------------------------------------------------------
def theta_rows64(theta):
    """The written-out pose map in the dtype of theta (closed form; theta = 0 is handled through a where)."""
    w = theta[:, :3]
    x = (w * w).sum(dim=1)
    zero = x == 0
    a = torch.where(zero, torch.ones_like(x), x).sqrt()
    ca = torch.where(zero, 1 - x / 6, torch.sin(a) / a)
    cb = torch.where(zero, 0.5 - x / 24, (1 - torch.cos(a)) / (a * a))
    o = torch.zeros_like(x)
    K = torch.stack([o, -w[:, 2], w[:, 1], w[:, 2], o, -w[:, 0], -w[:, 1], w[:, 0], o], dim=1).reshape(-1, 3, 3)
    R = torch.eye(3, dtype=theta.dtype) + ca[:, None, None] * K + cb[:, None, None] * (K @ K)
    s = theta[:, 6].exp()
    return torch.cat([torch.cat([s[:, None, None] * R, theta[:, 3:6, None]], dim=2).reshape(-1, 12), s[:, None]], dim=1)


def adam_reference(sd, pts, tgt, seg_off, z0, theta0, iters, lr, pose_lr, sigma, dtype, free=(True, True, True), cutoff=CUTOFF, watch=None):
    """(codes, theta, data term) after `iters` torch.optim.Adam steps over (z, theta) in `dtype`.  watch: a list that receives, per
    evaluation, the smallest distances to a kink: (min |pre-activation|, min |out - target'|, min ||ts target| - cutoff|)."""
    P = {k: v.to(dtype) for k, v in sd.items()}
    counts = seg_off[1:] - seg_off[:-1]
    sid = torch.repeat_interleave(torch.arange(counts.numel()), counts)
    z = z0.to(dtype).clone().requires_grad_(True)
    theta = theta0.to(dtype).clone().requires_grad_(True)
    mask = torch.tensor([float(free[0])] * 3 + [float(free[1])] * 3 + [float(free[2])], dtype=dtype)
    opt = torch.optim.Adam([{"params": [z], "lr": lr}, {"params": [theta], "lr": pose_lr}])
    p, t = pts.to(dtype), tgt.to(dtype)

    def data_term():
        x, ts = posed(theta_rows64(theta), sid, p)
        d = (O.sdfnet_forward(P, x, z[sid]).reshape(-1) - (ts * t).clamp(-cutoff, cutoff)).abs()
        if watch is not None:
            watch.append((float(O.sdfnet_min_preactivation(P, x.detach(), z.detach()[sid]).min()), float(d.detach().min()),
                          float(((ts * t).abs() - cutoff).abs().detach().min())))
        return torch.zeros(counts.numel(), dtype=dtype).index_add(0, sid, d) / counts.to(dtype)
    for _ in range(iters):
        opt.zero_grad()
        (data_term().sum() + sigma * (z * z).mean(dim=1).sum()).backward()
        theta.grad.mul_(mask)
        opt.step()
    return z.detach(), theta.detach(), data_term().detach()


# Ten Adam steps divide every gradient by its own running size, so one ReLU that two float32 evaluations take on different sides shows
# in the codes far above the criterion.  The inputs are therefore chosen (seed, by the float64 loop alone) so that no evaluation of the
# float64 trajectory comes closer to a kink than float32 can tell apart: 4 ulp of a float32 pre-activation of magnitude 0.5 (theirs are
# around 0.1) for ReLU, 1e-6 for the L1 loss and the clamp.  Few points, or no seed would do: about one pre-activation in 10^6 lies
# that close to zero, and an evaluation of N points has 1792 N of them.
FIT_RUNS = (40, 33, 5)
FIT_ITERS, FIT_LR, FIT_POSE_LR, FIT_SIGMA = 10, 1e-3, 1e-3, 0.01
FIT_SEED = 182
RELU_ALONG, L1_ALONG = 4 * 2.0 ** -23 * 0.5, 1e-6


def fit_inputs(seed, latent=64):
    sd = seeded_state(seed, latent)
    hidden = torch.randn(len(FIT_RUNS), latent, generator=torch.Generator().manual_seed(seed + 1)) * 0.5
    P64 = {k: v.double() for k, v in sd.items()}

    def target(points, s):      # the hidden code through the float64 net
        with torch.no_grad():
            return O.sdfnet_forward(P64, points, hidden[s:s + 1].double().expand(points.shape[0], -1)).reshape(-1) * 0.3
    ident = pose_rows_of("identity", len(FIT_RUNS), 0)
    pts, tgt, seg_off = safe_points(sd, torch.zeros_like(hidden), ident, list(FIT_RUNS), seed + 2, target=target)
    z0, th0 = torch.zeros(len(FIT_RUNS), latent), torch.zeros(len(FIT_RUNS), 7)
    return sd, (sd, pts, tgt, seg_off, z0, th0, FIT_ITERS, FIT_LR, FIT_POSE_LR, FIT_SIGMA)


def fit_margins(seed):
    """The float64 trajectory's smallest distances to a ReLU kink, to the L1 kink and to the clamp's."""
    watch = []
    _, args = fit_inputs(seed)
    adam_reference(*args, torch.float64, watch=watch)
    return tuple(min(w[i] for w in watch) for i in range(3))


@functools.lru_cache(maxsize=None)
def fit_case():
    latent, seed = 64, FIT_SEED
    sd, args = fit_inputs(seed, latent)
    watch = []
    r64 = adam_reference(*args, torch.float64, watch=watch)
    relu, l1, clamp = (min(w[i] for w in watch) for i in range(3))
    assert relu >= RELU_ALONG and l1 >= L1_ALONG and clamp >= L1_ALONG, "seed %d: the float64 trajectory passes a kink at %g / %g / %g" % (seed, relu, l1, clamp)
    return Case(sd=sd, seed=seed, latent=latent, pts=args[1], tgt=args[2], seg_off=args[3], r32=adam_reference(*args, torch.float32), r64=r64)


def body_fit(dev):
    """Ten Adam steps on "similarity" against float64 torch.optim.Adam over (z, theta); a shape fitted alone equals its row."""
    from shapegan_amd.reconstruct import fit_codes_and_poses
    case = fit_case()
    net = net_on(dev, case.seed, case.latent, case.sd)
    before = [p.detach().clone() for p in net.parameters()]
    kw = dict(iterations=FIT_ITERS, lr=FIT_LR, pose_lr=FIT_POSE_LR, sigma=FIT_SIGMA, cutoff=CUTOFF, pose="similarity")
    codes, poses, loss = fit_codes_and_poses(net, case.pts.to(dev), case.tgt.to(dev), case.seg_off.to(dev), **kw)
    check("pose fit", codes, case.r32[0], case.r64[0], "codes after %d Adam steps" % FIT_ITERS)
    check("pose fit", poses.theta, case.r32[1], case.r64[1], "theta after %d Adam steps" % FIT_ITERS)
    check("pose fit", loss, case.r32[2], case.r64[2], "returned loss")
    assert float(case.r64[1][:, :3].abs().min()) > 0 and float(case.r64[1][:, 6].abs().min()) > 0, "every group should have moved"
    for p, q in zip(net.parameters(), before):
        assert torch.equal(p.detach(), q) and p.grad is None, "the fit touched a parameter"
    so = case.seg_off.tolist()
    sl = slice(so[1], so[2])
    alone = fit_codes_and_poses(net, case.pts[sl].to(dev), case.tgt[sl].to(dev), points_per_shape=so[2] - so[1], **kw)
    assert torch.equal(alone[0][0].cpu(), codes[1].cpu()) and torch.equal(alone[1].theta[0].cpu(), poses.theta[1].cpu())
    assert torch.equal(alone[2][0].cpu(), loss[1].cpu())


def body_frozen_groups(dev, pose):
    """The groups a pose model does not free stay at their initial values, bit for bit; the free ones move."""
    from shapegan_amd.reconstruct import POSE_MODELS, Poses, fit_codes_and_poses
    case = fit_case()
    net = net_on(dev, case.seed, case.latent, case.sd)
    S = len(FIT_RUNS)
    th0 = torch.tensor([[0.1, -0.2, 0.05, 0.01, 0.02, -0.03, 0.1]] * S)
    init = Poses.from_theta(th0)
    _, poses, _ = fit_codes_and_poses(net, case.pts.to(dev), case.tgt.to(dev), case.seg_off.to(dev), iterations=3, pose=pose,
                                      pose_init=init, pose_lr=1e-2)
    start = poses_theta_of(init)
    got = poses.theta.cpu()
    for free, cols in zip(POSE_MODELS[pose], (slice(0, 3), slice(3, 6), slice(6, 7))):
        if free:
            assert bool((got[:, cols] != start[:, cols]).any(dim=1).all()), "%s: a free group did not move" % pose
        else:
            assert torch.equal(got[:, cols], start[:, cols]), "%s: a frozen group moved" % pose
    assert float((start - th0).abs().max()) < 1e-6, "pose_init should come back as the theta it was made from"


def poses_theta_of(init):
    """The theta a fit starts from for pose_init = init (one start)."""
    from shapegan_amd.reconstruct import _initial_theta
    return _initial_theta(len(init), 1, init, (0, 1, 0), "cpu")


# ---- recovery -------------------------------------------------------------------------------------------------------------------------
REC_POINTS, REC_ITERS, REC_LR, REC_POSE_LR = 400, 150, 1e-3, 2e-3
REC_AXIS, REC_ANGLE, REC_T, REC_S = (0.3, 0.8, -0.5), math.radians(10), 0.05, 1.1


def in_band_points(sd, codes, n, seed, band=0.08):
    """n points per shape with |f64| < band in the canonical frame, and the float64 values there."""
    g = torch.Generator().manual_seed(seed)
    P64 = {k: v.double() for k, v in sd.items()}
    pts, val = [], []
    for s in range(codes.shape[0]):
        kept, vals, have = [], [], 0
        while have < n:
            cand = (torch.rand(4000, 3, generator=g) * 1.6 - 0.8).double()
            zs = codes[s:s + 1].double().expand(cand.shape[0], -1)
            with torch.no_grad():
                out = O.sdfnet_forward(P64, cand, zs).reshape(-1)
            ok = (out.abs() < band) & ~fragile_points(sd, cand, zs, None)
            kept.append(cand[ok])
            vals.append(out[ok])
            have += int(ok.sum())
        pts.append(torch.cat(kept)[:n])
        val.append(torch.cat(vals)[:n])
    return torch.cat(pts), torch.cat(val)


def pose_errors(theta, R_true, t_true, s_true):
    """(rotation error in radians, translation error, |log scale error|) per shape of theta against the true canonical-from-observed map."""
    rows = theta_rows64(theta.double())
    M = rows[:, :12].reshape(-1, 3, 4)
    s = rows[:, 12]
    R = M[:, :, :3] / s[:, None, None]
    cosang = (((R.transpose(1, 2) @ R_true).diagonal(dim1=1, dim2=2).sum(dim=1) - 1) / 2).clamp(-1, 1)
    return torch.acos(cosang), (M[:, :, 3] - t_true).norm(dim=1), (s.log() - math.log(s_true)).abs()


@functools.lru_cache(maxsize=None)
def recovery_case(yaw_degrees=None, starts=1, iters=REC_ITERS):
    """Two chairs codes, 400 in-band points each with the float64 network's own values, observed through a known similarity: the map the
    fit should find is x = s R q + t.  With yaw_degrees the rotation is that yaw about +y instead (one shape is enough there)."""
    sd = chairs_state()
    latent = sd["layers1.0.weight"].shape[1] - 3
    S = 2
    codes = torch.randn(S, latent, generator=torch.Generator().manual_seed(7)) * 0.1
    x, val = in_band_points(sd, codes, REC_POINTS, 8)
    R = rodrigues(REC_AXIS, REC_ANGLE) if yaw_degrees is None else rodrigues((0, 1, 0), math.radians(yaw_degrees))
    t = torch.tensor([0.6, -0.64, 0.48], dtype=torch.float64) * REC_T      # |t| = 0.05
    # observed: q = R^T (x - t) / s, target distances in the observed frame: f / s
    q = ((x - t) @ R) / REC_S
    tgt = val / REC_S
    seg_off = segment_table([REC_POINTS] * S)[1]
    truth = (R.expand(S, 3, 3), t.expand(S, 3), REC_S)
    return Case(sd=sd, latent=latent, codes=codes, q=q, tgt=tgt, seg_off=seg_off, truth=truth, S=S, iters=iters)


def recovery_loop64(case, q, tgt, codes, theta0, iters):
    """The float64 loop (sigma = 0: the codes are given and true)."""
    return adam_reference(case.sd, q, tgt, case.seg_off, codes, theta0, iters, REC_LR, REC_POSE_LR, 0.0, torch.float64)


@functools.lru_cache(maxsize=None)
def recovery_reference():
    """e64 (the float64 loop's final errors, [3][S]), delta (their largest spread over three float64 runs on inputs rounded to float32
    and moved by one ulp) and the starting errors."""
    case = recovery_case()
    th0 = torch.zeros(case.S, 7, dtype=torch.float64)
    start = torch.stack(pose_errors(th0, *case.truth))
    _, th, _ = recovery_loop64(case, case.q, case.tgt, case.codes, th0, case.iters)
    e64 = torch.stack(pose_errors(th, *case.truth))
    assert bool((e64 < 0.1 * start).all()), "the float64 loop should cut every error below a tenth: %s -> %s" % (start, e64)
    runs = []
    g = torch.Generator().manual_seed(11)
    for k in range(3):
        q32 = case.q.float()
        if k:
            direction = torch.where(torch.rand(q32.shape, generator=g) < 0.5, torch.full_like(q32, float("inf")), torch.full_like(q32, -float("inf")))
            q32 = torch.nextafter(q32, direction)
        _, thk, _ = recovery_loop64(case, q32.double(), case.tgt.float().double(), case.codes.float(), th0, case.iters)
        runs.append(torch.stack(pose_errors(thk, *case.truth)))
    runs = torch.stack(runs)
    delta = (runs.max(dim=0).values - runs.min(dim=0).values).max(dim=1).values      # [3]: per kind of error
    return Case(e64=e64, delta=delta, start=start)


def body_recovery(dev):
    from shapegan_amd.reconstruct import fit_codes_and_poses
    case, ref = recovery_case(), recovery_reference()
    net = net_on(dev, 5, case.latent, case.sd)
    _, poses, _ = fit_codes_and_poses(net, case.q.float().to(dev), case.tgt.float().to(dev), case.seg_off.to(dev), iterations=case.iters,
                                      lr=REC_LR, pose_lr=REC_POSE_LR, sigma=0.0, init=case.codes, pose="similarity")
    got = torch.stack(pose_errors(poses.theta.cpu(), *case.truth))
    bound = 2 * ref.e64 + ref.delta[:, None]
    for name, g, b, e, st in zip(("rotation", "translation", "log scale"), got, bound, ref.e64, ref.start):
        print("[latent-pose] recovery %-11s start %s  e64 %s  delta %.3g  fused %s  bound %s" % (
            name, ["%.3g" % v for v in st.tolist()], ["%.3g" % v for v in e.tolist()], float(ref.delta[("rotation", "translation", "log scale").index(name)]),
            ["%.3g" % v for v in g.tolist()], ["%.3g" % v for v in b.tolist()]))
    assert bool((got <= bound).all()), "fused errors %s beyond 2 e64 + delta = %s" % (got, bound)


YAW_TRUE, YAW_STARTS, YAW_ITERS = 170.0, 4, 40


@functools.lru_cache(maxsize=None)
def yaw_reference():
    """The float64 loop from the four yaw starts: which start ends with the smallest data term, per shape."""
    case = recovery_case(YAW_TRUE, YAW_STARTS, YAW_ITERS)
    final = []
    for k in range(YAW_STARTS):
        th0 = torch.zeros(case.S, 7, dtype=torch.float64)
        th0[:, 1] = 2 * math.pi * k / YAW_STARTS
        final.append(recovery_loop64(case, case.q, case.tgt, case.codes, th0, YAW_ITERS)[2])
    best = torch.stack(final).argmin(dim=0)
    assert best.tolist() == [2] * case.S, "the float64 loop should keep the start at 180 degrees, the one nearest 170: %s" % best.tolist()
    return best


def body_rotation_starts(dev):
    """A true yaw of 170 degrees, four starts: float64 loop and fused fit keep the start nearest the truth (180 degrees)."""
    from shapegan_amd.reconstruct import fit_codes_and_poses
    case, best = recovery_case(YAW_TRUE, YAW_STARTS, YAW_ITERS), yaw_reference()
    net = net_on(dev, 5, case.latent, case.sd)
    _, poses, loss = fit_codes_and_poses(net, case.q.float().to(dev), case.tgt.float().to(dev), case.seg_off.to(dev), iterations=YAW_ITERS,
                                         lr=REC_LR, pose_lr=REC_POSE_LR, sigma=0.0, init=case.codes, pose="similarity",
                                         rotation_starts=YAW_STARTS)
    rot, _, _ = pose_errors(poses.theta.cpu(), *case.truth)
    assert poses.theta.shape == (case.S, 7) and loss.shape == (case.S,)
    assert bool((rot < math.radians(45)).all()), "the kept start is not the one nearest 170 degrees: rotation errors %s" % rot
    yaw = poses.theta.cpu()[:, 1].abs()
    assert bool(((yaw - math.pi * best.double() / 2).abs() < math.radians(45)).all())


# ---- surface ------------------------------------------------------------------------------------------------------------------------
def body_meshes(dev):
    """reconstruct_meshes(poses=None) is today's batch bit for bit; with poses the vertices are to_observed of the canonical ones and
    the normals stay unit; Poses round-trips and saves."""
    import os
    import tempfile
    from shapegan_amd.reconstruct import Poses, reconstruct_meshes
    sd = chairs_state()
    latent = sd["layers1.0.weight"].shape[1] - 3
    net = net_on(dev, 5, latent, sd)
    codes = (torch.randn(2, latent, generator=torch.Generator().manual_seed(17)) * 0.1).to(dev)
    plain = reconstruct_meshes(net, codes, voxel_resolution=16)
    none = reconstruct_meshes(net, codes, voxel_resolution=16, poses=None)
    assert int(plain.faces.shape[0]) > 0
    for name in ("vertices", "normals", "faces", "vert_offsets", "tri_offsets"):
        assert torch.equal(getattr(plain, name), getattr(none, name)), name
    poses = Poses.from_theta(torch.tensor([[0.2, -0.1, 0.3, 0.05, 0.0, -0.02, 0.1], [0.0, 0.5, 0.0, 0.0, 0.1, 0.0, -0.2]]).to(dev))
    moved = reconstruct_meshes(net, codes, voxel_resolution=16, poses=poses)
    assert torch.equal(moved.faces, plain.faces) and torch.equal(moved.vert_offsets, plain.vert_offsets)
    vo = plain.vert_offsets.tolist()
    for s in range(2):
        sl = slice(vo[s], vo[s + 1])
        assert torch.equal(moved.vertices[sl], poses.to_observed(plain.vertices[sl], s)), "shape %d: vertices" % s
        back = poses.to_canonical(moved.vertices[sl], s)
        assert float((back - plain.vertices[sl]).abs().max()) < 1e-5, "to_canonical does not undo to_observed"
        n0, n1 = plain.normals[sl], moved.normals[sl]
        unit = n0.norm(dim=1) > 0.5
        assert float((n1[unit].norm(dim=1) - 1).abs().max()) < 1e-5, "shape %d: the normals are no longer unit" % s
        R = poses.matrix[s, :, :3] / poses.scale[s]
        assert float((n1 @ R.T - n0).abs().max()) < 1e-5
    with pytest.raises(ValueError, match="poses for"):
        reconstruct_meshes(net, codes[:1], voxel_resolution=16, poses=poses)
    with tempfile.TemporaryDirectory() as d:
        poses.save(os.path.join(d, "poses.to"))
        raw = torch.load(os.path.join(d, "poses.to"))
        assert sorted(raw) == ["matrix", "scale"] and all(torch.is_tensor(v) for v in raw.values())
        again = Poses.load(os.path.join(d, "poses.to"))
    assert torch.equal(again.matrix, poses.matrix.cpu()) and torch.equal(again.scale, poses.scale.cpu())
    assert again.matrix.shape == (2, 3, 4) and again.scale.shape == (2,)


def body_cli(tmp_path, capsys):
    """The command line on the two-tetrahedron .obj of the latent fit's test, on the CPU: with --pose translation+scale --poses-out the
    poses are saved and have the identity's rotation; without --pose it prints what fit_latent_codes' command line prints."""
    from latent_fit_forms import TETRAHEDRA
    from shapegan_amd import reconstruct
    models = tmp_path / "models" / "abc" / "models"
    models.mkdir(parents=True)
    (models / "model_normalized.obj").write_text(TETRAHEDRA)
    torch.save(chairs_state(), str(tmp_path / "sdf_net.to"))
    common = ["--net", str(tmp_path / "sdf_net.to"), "--models", str(tmp_path / "models"), "--meshes", str(tmp_path / "meshes"), "--chamfer",
              "--device", "cpu", "--points", "300", "--iterations", "2", "--scan-count", "6", "--scan-resolution", "64", "--resolution", "16",
              "--chamfer-points", "64"]
    assert reconstruct.main(common + ["--out", str(tmp_path / "plain.to")]) == 0
    plain_text = capsys.readouterr().out
    plain = torch.load(str(tmp_path / "plain.to"))
    # today's output: one line per model, "<path>: loss <6 decimals>, chamfer <6 decimals | n/a>", and nothing about poses
    line = r"\S*model_normalized\.obj: loss \d+\.\d{6}( \(bad mesh: too little inside\))?, chamfer (\d+\.\d{6}|n/a \(empty reconstruction\))"
    assert re.fullmatch(line, plain_text.strip()), plain_text
    assert plain.shape == (1, 128) and float(plain.abs().max()) > 0
    poses_file = tmp_path / "out" / "poses.to"
    rc = reconstruct.main(common + ["--out", str(tmp_path / "posed.to"), "--pose", "translation+scale", "--poses-out", str(poses_file),
                                    "--pose-lr", "0.01"])
    assert rc == 0
    text = capsys.readouterr().out
    assert "model_normalized.obj: loss" in text and "chamfer" in text
    poses = reconstruct.Poses.load(str(poses_file))
    assert poses.matrix.shape == (1, 3, 4) and poses.scale.shape == (1,)
    s = float(poses.scale[0])
    assert s != 1.0 and abs(s - 1.0) < 0.1 and float(poses.matrix[0, :, 3].abs().max()) > 0
    assert torch.equal(poses.matrix[0, :, :3], torch.eye(3) * poses.scale[0]), "translation+scale leaves the rotation at the identity"
    assert (tmp_path / "meshes" / "0000.obj").exists()
    for alone in (["--poses-out", str(poses_file)], ["--pose-starts", "2"], ["--pose-lr", "0.01"]):
        with pytest.raises(SystemExit):
            reconstruct.main(common + ["--out", str(tmp_path / "x.to")] + alone)
