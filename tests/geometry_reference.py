"""Float64 references and shared cases for the render (csrc/raymarch.hip) and mesh (csrc/mesh.hip) kernels, stage by stage.

Everything here is written from the contracts in include/shapegan_hip.h (the K12 and sphere-tracing comment blocks) in
numpy / torch float64 and shares no code with the kernels or with the C++ twin.  The test bodies take a device: the CPU tier
(tests/test_render_stages.py, tests/test_mesh_reference.py) runs them on the twin, the GPU tier (tests/test_gpu_render_stages.py,
tests/test_gpu_mesh.py) on the MI355X.  Every body returns the figures it measured (maxima, fragile shares) next to asserting
the bounds; DESIGN.md 3.7 / 3.8 record them.

Tolerances (none of them comes from the code under test):
  U = 2^-24, the relative error of one float32 rounding.
  march: SDF_ATOL = 2e-6 is the project's bound for the fused SDFNet forward (tests/test_gpu_ops.py::test_sdfnet_points_mode); a
         position may differ by that times |dir| <= 1 plus two float32 ulps of the coordinate; a ray whose SDF value (or |p|, or
         y) lies within that band of a decision point is fragile and may classify either way.
"""
import ctypes
import importlib.util
import math
import os

import numpy as np
import torch

from oracle import torch_oracle as O
from shapegan_amd import ops
from shapegan_amd.lib import check, ptr, stream
from shapegan_amd.rendering import raymarching as rm

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24
SDF_ATOL = 2e-6
MARCH_FRAGILE_CAP = 1e-3
GROUND_FRAGILE_CAP = 1e-3
SAMPLE_FRAGILE_CAP = 1e-4


def f32(x):
    """The float32 value a kernel receives for the Python float x, as a float64."""
    return float(np.float32(x))


def ulp32(x):
    """One float32 ulp at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def doubles(values):
    values = [float(v) for v in values]
    return (ctypes.c_double * len(values))(*values)


def npy(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------
# camera rays (sg_raymarch_rays)
# ------------------------------------------------------------------------------------------------------------------------
def camera(focal_radius):
    """The 13 doubles of the header: position, right, up, forward, focal distance (for a sphere of focal_radius in view)."""
    p = np.asarray(rm.camera_position, dtype=np.float64)
    fwd = -p / np.linalg.norm(p)
    right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    up /= np.linalg.norm(up)
    focal = 1.0 / math.tan(math.asin(focal_radius / float(np.linalg.norm(p))))
    return np.concatenate([p, right, up, fwd, [focal]])


def rays_reference(cam, W, radius):
    """dirs [M,3] float32 (bit pattern expected), start positions [M,3] float64, enters [M] bool, fragile [M] bool."""
    xs = np.linspace(-1.0, 1.0, W)
    X, Y = np.meshgrid(xs, xs)            # x along a row, y down the rows
    sx, sy = X.reshape(-1, 1), Y.reshape(-1, 1)
    d = (sx * cam[3:6] + sy * cam[6:9] + cam[12] * cam[9:12]).astype(np.float32)      # the one cast of the header
    n = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    d = d / n[:, None]
    p32 = cam[0:3].astype(np.float32)
    b = (p32[0] * d[:, 0] + p32[1] * d[:, 1] + p32[2] * d[:, 2]) * np.float32(2)
    c = float(np.dot(cam[0:3], cam[0:3])) - radius * radius
    bb = (b * b).astype(np.float64)
    disc = bb - 4.0 * c
    enters = disc >= 0
    # b carries a few float32 roundings: a discriminant within them of 0 may fall either way
    fragile = np.abs(disc) <= 8 * U * bb
    t = (-b.astype(np.float64) - np.sqrt(np.where(enters, disc, 0.0))) / 2
    pos = np.where(enters[:, None], p32.astype(np.float64) + d.astype(np.float64) * t[:, None], p32.astype(np.float64))
    return d, pos, enters, fragile


def run_rays(dev, cam, W, S, radius):
    M = W * W
    dirs = torch.empty((M, 3), dtype=torch.float32, device=dev)
    pos = torch.empty((S * M, 3), dtype=torch.float32, device=dev)
    status = torch.full((S * M,), 7, dtype=torch.uint8, device=dev)
    active = torch.full((2 * S * M,), -1, dtype=torch.int32, device=dev)
    counts = torch.zeros(3 * S, dtype=torch.int32, device=dev)
    check(ops._lib().sg_raymarch_rays(doubles(cam), W, S, float(radius), ptr(dirs), ptr(pos), ptr(status), ptr(active), ptr(counts),
                                      stream()), "raymarch_rays")
    return dirs, pos, status, active, counts


def check_rays(dev, W, S, radius, focal_radius):
    cam = camera(focal_radius)
    M = W * W
    dirs, pos, status, active, counts = run_rays(dev, cam, W, S, radius)
    d_ref, p_ref, enters, fragile = rays_reference(cam, W, radius)
    assert int(fragile.sum()) <= 4, "more than a handful of pixels at the sphere's rim: %d" % int(fragile.sum())
    assert np.array_equal(npy(dirs).view(np.int32), d_ref.view(np.int32)), "dirs are not bit-equal"
    assert not npy(status).any()
    pos, active, counts = npy(pos).astype(np.float64).reshape(S, M, 3), npy(active)[:S * M].reshape(S, M), npy(counts)
    ok = ~fragile
    err = np.abs(pos[:, ok] - p_ref[None, ok])
    assert (err <= 2 * ulp32(p_ref[None, ok])).all(), err.max()
    assert not counts[S:].any()
    want = np.flatnonzero(enters & ok)
    for s in range(S):
        lst = active[s, :counts[s]]
        assert len(np.unique(lst)) == len(lst)
        got = lst - s * M
        assert ((got >= 0) & (got < M)).all()
        sure = got[ok[got]]
        assert np.array_equal(np.sort(sure), want), s
        assert counts[s] == len(want) + int(fragile[got].sum())
    return dict(entering=int(enters.sum()), fragile=int(fragile.sum()), pos_err=float(err.max()) if err.size else 0.0)


RAY_CASES = [(W, S) for W in (1, 2, 3, 16, 37, 100) for S in (1, 3)] + [(1, 128), (3, 128), (37, 128)]
# (sphere radius, radius the focal distance is made for): the renderer's own pairs, a sphere so small that the corner (and most
# other) rays miss it, and a field of view so narrow that every ray enters
RAY_RADII = [(1.0, 1.0), (1.6, 1.6), (0.5, 1.6), (1.6, 0.7)]


# ------------------------------------------------------------------------------------------------------------------------
# march steps (sg_raymarch_steps / sg_raymarch_finish)
# ------------------------------------------------------------------------------------------------------------------------
class March(object):
    """The buffers of one march on `dev` and the raw entry points on them."""

    def __init__(self, net, z, pos, dirs, dir_period, lists, nshapes, clamp, threshold, offset, radius0, radius1, shadow):
        dev = pos.device
        self.net, self.z, self.dev = net, z, dev
        self.packed, self.zb1, self.zb5 = net._pack_shapes.get_with_fold(net._params(), z)
        self.pos, self.dirs, self.dir_period = pos.contiguous().clone(), dirs.contiguous(), int(dir_period)
        self.nrays, self.nseg, self.nshapes = pos.shape[0], len(lists), int(nshapes)
        sizes = [len(x) for x in lists]
        # a segment's list lives at seg_off[seg]: give every segment the room of its first list
        self.seg_off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
        assert int(self.seg_off[-1]) <= self.nrays
        self.status = torch.zeros(self.nrays, dtype=torch.uint8, device=dev)
        act = np.full(2 * self.nrays, -1, dtype=np.int32)
        for s, l in enumerate(lists):
            act[int(self.seg_off[s]):int(self.seg_off[s]) + len(l)] = l
        self.active = torch.from_numpy(act).to(dev)
        cnt = np.zeros(3 * self.nseg, dtype=np.int32)
        cnt[:self.nseg] = sizes
        self.counts = torch.from_numpy(cnt).to(dev)
        self.evals = torch.zeros(1, dtype=torch.int64, device=dev)
        self.par = dict(clamp=clamp, threshold=threshold, offset=offset, radius0=radius0, radius1=radius1, shadow=int(shadow))
        self.iter = 0

    def clone(self):
        m = object.__new__(March)
        m.__dict__.update(self.__dict__)
        for k in ("pos", "status", "active", "counts", "evals"):
            setattr(m, k, getattr(self, k).clone())
        return m

    def steps(self, k, max_rays=None):
        p = self.par
        check(ops._lib().sg_raymarch_steps(ptr(self.packed), ptr(self.zb1), ptr(self.zb5), ptr(self.pos), ptr(self.dirs),
                                           self.dir_period, ptr(self.status), ptr(self.active), self.nrays, ptr(self.counts),
                                           ptr(self.seg_off), self.nseg, self.nshapes, self.nrays if max_rays is None else max_rays,
                                           self.iter, k, p["clamp"], p["threshold"], p["offset"], p["radius0"], p["radius1"],
                                           p["shadow"], ptr(self.evals), stream()), "raymarch_steps")
        self.iter += k

    def finish(self):
        check(ops._lib().sg_raymarch_finish(ptr(self.status), ptr(self.active), self.nrays, ptr(self.counts), ptr(self.seg_off),
                                            self.nseg, self.iter, stream()), "raymarch_finish")

    def lists(self, it=None):
        """The list of every segment before step `it` (numpy), whatever its count."""
        it = self.iter if it is None else it
        act = npy(self.active)[(it & 1) * self.nrays:][:self.nrays]
        cnt = npy(self.counts).reshape(3, self.nseg)[it % 3]
        off = npy(self.seg_off)
        return [act[off[s]:off[s] + cnt[s]].copy() for s in range(self.nseg)]

    def live_total(self):
        cnt = npy(self.counts).reshape(3, self.nseg)[self.iter % 3]
        return int(cnt[(cnt >= 2) | (self.iter == 0)].sum())


def sdfnet64(state64, z64, points, shape_of_point):
    with torch.no_grad():
        out = O.sdfnet_forward(state64, torch.from_numpy(points), z64[torch.from_numpy(shape_of_point)])
    return out.reshape(-1).numpy()


def lockstep_step(m, state64, z64):
    """One step of `m` against the float64 reference computed from m's own state before the step.  Returns
    (rays marched, fragile rays, largest position error)."""
    p = m.par
    it = m.iter
    pos0, status0, evals0 = npy(m.pos).copy(), npy(m.status).copy(), int(m.evals.item())
    cur = m.lists()
    live = [s for s in range(m.nseg) if len(cur[s]) >= 2 or (it == 0 and len(cur[s]) > 0)]
    lone = [int(cur[s][0]) for s in range(m.nseg) if it > 0 and len(cur[s]) == 1]
    rays = np.concatenate([cur[s] for s in live]).astype(np.int64) if live else np.zeros(0, dtype=np.int64)
    segs = np.concatenate([np.full(len(cur[s]), s) for s in live]).astype(np.int64) if live else np.zeros(0, dtype=np.int64)
    assert len(np.unique(rays)) == len(rays)
    assert not status0[rays].any(), "an active ray is already marked"

    m.steps(1)

    pos1, status1 = npy(m.pos), npy(m.status)
    nxt = m.lists()
    counts = npy(m.counts).reshape(3, m.nseg)
    assert not counts[(it + 2) % 3].any(), "the counts of iteration iter + 2 are not zero"
    assert int(m.evals.item()) - evals0 == len(rays)
    # rays that were not marched: untouched bit for bit, but for the last ray of a finished segment, which is now a hit
    rest = np.ones(m.nrays, dtype=bool)
    rest[rays] = False
    assert np.array_equal(pos1[rest].view(np.int32), pos0[rest].view(np.int32))
    want = status0.copy()
    want[lone] = 1
    assert np.array_equal(status1[rest], want[rest])
    for s in range(m.nseg):
        if s not in live:
            assert len(nxt[s]) == 0, "a finished segment was marched again"
    if len(rays) == 0:
        return 0, 0, 0.0

    # the reference step, from the state before it
    x = pos0[rays].astype(np.float64)
    dirs = npy(m.dirs).astype(np.float64)
    d = dirs[rays % m.dir_period if m.dir_period > 0 else rays]
    u = sdfnet64(state64, z64, x, segs % m.nshapes) + f32(p["offset"])
    cl, th = f32(p["clamp"]), f32(p["threshold"])
    sd = np.clip(u, -cl, cl)
    ref = x + d * sd[:, None]
    hit = (sd > 0) & (sd < th)
    radius = np.where(segs < m.nshapes, f32(p["radius0"]), f32(p["radius1"]))
    reach = ref[:, 1] if p["shadow"] else np.linalg.norm(ref, axis=1)
    miss = reach > radius
    fragile = (np.abs(u) < SDF_ATOL) | (np.abs(u - th) < SDF_ATOL) | (np.abs(np.abs(u) - cl) < SDF_ATOL)
    fragile |= np.abs(reach - radius) < SDF_ATOL + 2 * ulp32(radius)
    survive = ~hit & ~miss

    got = pos1[rays].astype(np.float64)
    err = np.abs(got - ref)
    bound = SDF_ATOL + 2 * ulp32(ref)          # SDF_ATOL times |dir| <= 1, plus two ulps of the coordinate
    assert (err <= bound).all(), ("position", float((err - bound).max()), float(err.max()))
    sure = ~fragile
    assert np.array_equal(status1[rays][sure] != 0, hit[sure]), "newly set status bytes differ from the hits"
    assert (status1[rays] <= 1).all()
    in_next = np.zeros(m.nrays, dtype=bool)
    for s in live:
        lst = nxt[s]
        assert len(np.unique(lst)) == len(lst), "duplicates in the next list"
        assert np.isin(lst, cur[s]).all(), "the next list holds a ray of another segment"
        in_next[lst] = True
    assert np.array_equal(in_next[rays][sure], survive[sure]), "the next lists differ from the survivors"
    assert not (in_next[rays] & (status1[rays] != 0)).any(), "a hit ray survives"
    return len(rays), int(fragile.sum()), float(err.max())


def lockstep(m, state, steps):
    """Marches `steps` steps (or until nothing is live) in lockstep; returns dict(ray_steps, fragile, pos_err, outcomes)."""
    state64 = {k: v.double() for k, v in state.items()}
    z64 = m.z.detach().cpu().double()
    total = frag = 0
    worst = 0.0
    lone_seen = 0
    for _ in range(steps):
        if m.iter > 0:
            lone_seen += sum(1 for l in m.lists() if len(l) == 1)
        n, f, e = lockstep_step(m, state64, z64)
        total, frag, worst = total + n, frag + f, max(worst, e)
        if n == 0 and m.iter > 1:
            break
    assert frag <= MARCH_FRAGILE_CAP * max(total, 1), (frag, total)
    return dict(ray_steps=total, fragile=frag, pos_err=worst, steps=m.iter, lone_segments=lone_seen)


def latents(golden_latents, n, seed=5):
    """The golden latents first, then seeded ones of the same scale."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((n, golden_latents.shape[1]), generator=g) * 0.5
    k = min(n, golden_latents.shape[0])
    z[:k] = torch.from_numpy(golden_latents[:k])
    return z


def camera_march(net, golden_latents, W=24, nz=3, radius=1.6, offset=-0.045, threshold=0.0005):
    """Case (a): the renderer's camera march, dir_period = M, shadow = 0."""
    dev = net.device
    z = latents(golden_latents, nz).to(dev)
    dirs, pos, status, active, counts = run_rays(dev, camera(radius), W, nz, radius)
    M = W * W
    act, cnt = npy(active), npy(counts)
    lists = [act[s * M:s * M + cnt[s]] for s in range(nz)]
    m = March(net, z, pos, dirs, M, [np.arange(s * M, (s + 1) * M) for s in range(nz)], nz, 0.02, threshold, offset, radius, radius, 0)
    # (every segment owns M slots; only the entering rays are listed)
    a = np.full(2 * m.nrays, -1, dtype=np.int32)
    for s in range(nz):
        a[s * M:s * M + cnt[s]] = lists[s]
    m.active = torch.from_numpy(a).to(dev)
    c = np.zeros(3 * nz, dtype=np.int32)
    c[:nz] = cnt[:nz]
    m.counts = torch.from_numpy(c).to(dev)
    return m


SHADOW_SIZES = (0, 1, 2, 3, 63, 64, 65, 200)


def shadow_segment_sizes(seed=9):
    """256 segment sizes: draws from SHADOW_SIZES, a stretch of 0- / 1- / 2-ray segments (a 64-ray tile straddles up to 64 of
    them), three of a few hundred (tiles wholly inside one segment)."""
    rng = np.random.RandomState(seed)
    sizes = rng.choice(SHADOW_SIZES, size=256, p=[0.15, 0.15, 0.15, 0.2, 0.1, 0.1, 0.1, 0.05])
    sizes[96:176] = rng.choice([0, 1, 1, 1, 1, 2], size=80)
    sizes[100:164] = 1
    sizes[[7, 130 + 70, 255]] = (300, 257, 513)
    return sizes.astype(np.int64)


def shadow_march(net, golden_latents, seed=9):
    """Case (b): dir_period = 0, shadow = 1, two radii, 128 shapes in 256 segments of every awkward size."""
    dev = net.device
    rng = np.random.RandomState(seed)
    sizes = shadow_segment_sizes(seed)
    n = int(sizes.sum())
    z = latents(golden_latents, 128).to(dev)
    # start points inside the unit ball, directions in the upper half space (toward a light): rays leave through y > radius,
    # meet the shape, or keep going
    x = rng.normal(size=(n, 3))
    x *= (rng.uniform(size=(n, 1)) ** (1 / 3)) * 0.9 / np.linalg.norm(x, axis=1, keepdims=True)
    perm = rng.permutation(n)       # the lists name rays all over the buffers
    off = np.concatenate([[0], np.cumsum(sizes)])
    # ... but outside the shapes: a ray that starts inside creeps up to the surface from below, its SDF value tends to 0 and never
    # counts as a hit, and every such ray ends up fragile.  (Chosen with the float64 network, not with the code under test.)
    state64 = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    shape = np.zeros(n, dtype=np.int64)
    shape[perm] = np.repeat(np.arange(256), sizes) % 128
    for _ in range(6):
        inside = sdfnet64(state64, z.detach().cpu().double(), x, shape) - 0.045 < 0.01
        y = rng.normal(size=(n, 3))
        y *= (rng.uniform(size=(n, 1)) ** (1 / 3)) * 0.9 / np.linalg.norm(y, axis=1, keepdims=True)
        x[inside] = y[inside]
    d = rng.normal(size=(n, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.3
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d32 = d.astype(np.float32)
    d32 /= np.maximum(np.linalg.norm(d32.astype(np.float64), axis=1, keepdims=True), 1.0).astype(np.float32)   # |dir| <= 1
    lists = [perm[off[s]:off[s + 1]].astype(np.int32) for s in range(256)]
    return March(net, z, torch.from_numpy(x.astype(np.float32)).to(dev), torch.from_numpy(d32).to(dev), 0, lists, 128, 0.1, 0.001,
                 -0.045, 1.6, 1.0, 1)


def assert_same_march(a, b):
    assert a.iter == b.iter
    assert torch.equal(a.pos.view(torch.int32), b.pos.view(torch.int32)), "pos"
    assert torch.equal(a.status, b.status), "status"
    assert torch.equal(a.counts, b.counts), "counts"
    assert torch.equal(a.evals, b.evals), "evals"
    for s, (la, lb) in enumerate(zip(a.lists(), b.lists())):
        assert np.array_equal(np.sort(la), np.sort(lb)), ("list", s)


def check_chunking(start, repeat=False):
    """Case (c): 16 steps as 16 calls, as one call, and as 7 + 9 with first_iter carried; max_rays = nrays and = the live total."""
    one = start.clone()
    for _ in range(16):
        one.steps(1)
    whole = start.clone()
    whole.steps(16)
    assert_same_march(one, whole)
    split = start.clone()
    split.steps(7, max_rays=split.live_total())
    split.steps(9, max_rays=split.live_total())
    assert_same_march(one, split)
    tight = start.clone()
    for _ in range(16):
        tight.steps(1, max_rays=tight.live_total())
    assert_same_march(one, tight)
    if repeat:
        again = start.clone()
        again.steps(16)
        assert_same_march(whole, again)
    return one


def check_finish(m):
    """Case (d): sg_raymarch_finish marks exactly the rays of the current lists."""
    before = npy(m.status).copy()
    pos = npy(m.pos).copy()
    listed = np.concatenate(m.lists()).astype(np.int64)
    assert len(listed) > 0, "the cap must stop a march that still has rays"
    f = m.clone()
    f.finish()
    want = before.copy()
    want[listed] = 1
    assert np.array_equal(npy(f.status), want)
    assert np.array_equal(npy(f.pos).view(np.int32), pos.view(np.int32))
    assert torch.equal(f.counts, m.counts) and torch.equal(f.active, m.active)
    return len(listed), int(want.sum() - before.sum())


def shadows_reference(state, z, points, light, threshold, offset, radius):
    """get_shadows for a handful of points in float64, free running (no lockstep): (status [n], fragile)."""
    state64 = {k: v.double() for k, v in state.items()}
    z64 = z.detach().cpu().double().reshape(1, -1)
    n = points.shape[0]
    d = light[None, :] - points
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32).astype(np.float64)
    x = points.astype(np.float32).astype(np.float64) + d * f32(0.1)
    x = x.astype(np.float32).astype(np.float64)
    status = np.zeros(n, dtype=np.float32)
    act = np.arange(n)
    fragile = False
    th, cl, r = f32(threshold), f32(0.1), f32(radius)
    for it in range(200):
        if len(act) == 0 or (it > 0 and len(act) < 2):
            break
        u = sdfnet64(state64, z64, x[act], np.zeros(len(act), dtype=np.int64)) + f32(offset)
        sd = np.clip(u, -cl, cl)
        x[act] = (x[act] + d[act] * sd[:, None]).astype(np.float32).astype(np.float64)
        hit = (sd > 0) & (sd < th)
        miss = x[act, 1] > r
        band = SDF_ATOL * (it + 1) * 4
        fragile |= bool(((np.abs(u) < band) | (np.abs(u - th) < band) | (np.abs(x[act, 1] - r) < band)).any())
        status[act[hit]] = 1
        act = act[~hit & ~miss]
    status[act] = 1       # fewer than 2 left, or the cap: the rest is shadowed
    return status, fragile


# ------------------------------------------------------------------------------------------------------------------------
# hits, ground plane, shadow-ray setup (sg_raymarch_classify / sg_raymarch_emit) and shading (sg_raymarch_shade)
# ------------------------------------------------------------------------------------------------------------------------
def scene_inputs(M, S, seed):
    """Random unit directions, positions in +-1.6 and status bytes; image 1 has no hit, image 3 exactly one, image 4 only hits."""
    rng = np.random.RandomState(seed)
    d = rng.normal(size=(M, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = rng.uniform(-1.6, 1.6, size=(S, M, 3))
    status = (rng.uniform(size=(S, M)) < 0.3).astype(np.uint8) * rng.choice([1, 1, 255], size=(S, M)).astype(np.uint8)
    if S > 1:
        status[1] = 0
    if S > 3:
        status[3] = 0
        status[3, M // 3] = 1
        pos[3, M // 3, 1] = 0.25      # (inside every cutoff used)
    if S > 4:
        status[4] = 1
    return d.astype(np.float32), pos.astype(np.float32).reshape(S * M, 3), status.reshape(S * M)


def run_scene(dev, dirs, pos, status, M, S, use_cutoff, vcut):
    lib = ops._lib()
    dirs_t, pos_t, status_t = (torch.from_numpy(a).to(dev) for a in (dirs, pos, status.copy()))
    ws = torch.empty(max(1, lib.sg_raymarch_workspace_bytes(M, S)), dtype=torch.uint8, device=dev)
    ground = torch.full((S,), -7.0, dtype=torch.float32, device=dev)
    offs = torch.full((2, S + 1), -1, dtype=torch.int64, device=dev)
    check(lib.sg_raymarch_classify(ptr(status_t), ptr(pos_t), ptr(dirs_t), M, S, int(use_cutoff), float(vcut), ptr(ground),
                                   ptr(offs[0]), ptr(offs[1]), ptr(ws), ws.numel(), stream()), "raymarch_classify")
    offs_h = npy(offs)
    H, G = int(offs_h[0, S]), int(offs_h[1, S])
    NS = max(H + G, 1)
    out = dict(hit_pos=torch.zeros((max(H, 1), 3), dtype=torch.float32, device=dev),
               hit_sid=torch.full((max(H, 1),), -1, dtype=torch.int32, device=dev),
               slot=torch.full((S * M,), -9, dtype=torch.int32, device=dev),
               spos=torch.zeros((NS, 3), dtype=torch.float32, device=dev), sdir=torch.zeros((NS, 3), dtype=torch.float32, device=dev),
               sactive=torch.full((2 * NS,), -1, dtype=torch.int32, device=dev),
               scounts=torch.full((6 * S,), -1, dtype=torch.int32, device=dev),
               sseg=torch.full((2 * S + 1,), -1, dtype=torch.int64, device=dev))
    light = np.asarray(rm.light_position, dtype=np.float64)
    check(lib.sg_raymarch_emit(ptr(status_t), ptr(pos_t), ptr(dirs_t), M, S, ptr(ground), ptr(offs[0]), ptr(offs[1]), doubles(light),
                               ptr(out["hit_pos"]), ptr(out["hit_sid"]), ptr(out["slot"]), ptr(out["spos"]), ptr(out["sdir"]),
                               ptr(out["sactive"]), ptr(out["scounts"]), ptr(out["sseg"]), ptr(ws), ws.numel(), stream()),
          "raymarch_emit")
    res = {k: npy(v) for k, v in out.items()}
    res.update(status=npy(status_t), ground=npy(ground), hit_off=offs_h[0], gnd_off=offs_h[1], H=H, G=G, light=light,
               tensors=dict(out, dirs=dirs_t))
    return res


def check_scene(dev, M, S, use_cutoff, vcut=0.8, seed=3):
    dirs, pos, status = scene_inputs(M, S, seed)
    r = run_scene(dev, dirs, pos, status, M, S, use_cutoff, vcut)
    light = r["light"]
    y = pos[:, 1]
    hit = status != 0
    if use_cutoff:
        hit &= ~((y > np.float32(vcut)) | (y < -np.float32(vcut)))
    assert np.array_equal(r["status"] != 0, hit)
    assert np.array_equal(r["status"][hit], status[hit]), "a kept status byte changed"
    hit2 = hit.reshape(S, M)
    nh = hit2.sum(axis=1)
    hit_off = np.concatenate([[0], np.cumsum(nh)])
    assert np.array_equal(r["hit_off"], hit_off)
    H = int(hit_off[-1])
    ground = np.array([y.reshape(S, M)[s][hit2[s]].min() if nh[s] else np.inf for s in range(S)], dtype=np.float32)
    assert np.array_equal(r["ground"].view(np.int32), ground.view(np.int32)), (r["ground"], ground)
    if S > 1:
        assert nh[1] == 0 and r["ground"][1] == np.inf       # the minimum over nothing
    if S > 4:
        assert nh[3] == 1 and (nh[4] == M or use_cutoff)
    # ground rays in float64
    p64, d64 = pos.astype(np.float64).reshape(S, M, 3), dirs.astype(np.float64)
    down = d64[:, 1] < 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = (p64[:, :, 1] - ground.astype(np.float64)[:, None]) / d64[None, :, 1]
        q = p64 - d64[None] * t[:, :, None]
        rxz = np.sqrt(q[:, :, 0] ** 2 + q[:, :, 2] ** 2)
    cand = down[None, :] & ~hit2 & (nh > 0)[:, None]
    gnd = cand & (rxz < 3)
    fragile = cand & (np.abs(rxz - 3) < 1e-5)
    assert fragile.sum() <= GROUND_FRAGILE_CAP * S * M, fragile.sum()
    slot = r["slot"].reshape(S, M)
    gnd = np.where(fragile, slot <= -2, gnd)     # a fragile pixel may fall either way: take the side the code took
    ng = gnd.sum(axis=1)
    gnd_off = np.concatenate([[0], np.cumsum(ng)])
    assert np.array_equal(r["gnd_off"], gnd_off)
    G = int(gnd_off[-1])
    want = np.full(S * M, -1, dtype=np.int64)
    want[hit] = np.arange(H)
    want[gnd.reshape(-1)] = -2 - np.arange(G)
    assert np.array_equal(r["slot"], want), "slot"
    assert np.array_equal(r["hit_pos"][:H].view(np.int32), pos[hit].view(np.int32))
    assert np.array_equal(r["hit_sid"][:H], np.repeat(np.arange(S), nh))
    # shadow rays: [0, H) from the hits, [H, H + G) from the ground points
    start = np.concatenate([p64.reshape(-1, 3)[hit], q.reshape(-1, 3)[gnd.reshape(-1)]])
    # magnitude of the float32 terms behind a start coordinate: the hit position, or p, d t and q of the ground point
    mag = np.concatenate([np.abs(p64.reshape(-1, 3)[hit]),
                          (np.abs(p64) + np.abs(d64[None] * t[:, :, None]) + np.abs(q)).reshape(-1, 3)[gnd.reshape(-1)]])
    dl = light[None, :] - start
    dl /= np.linalg.norm(dl, axis=1, keepdims=True)
    # direction: computed in double and cast (one float32 rounding, |d| <= 1) — for a ground point on top of the float32 error
    # of q (six roundings: subtract, divide, multiply, subtract per coordinate and their inputs) seen from >= 3 away
    far = np.linalg.norm(light[None, :] - start, axis=1, keepdims=True)
    derr = np.abs(r["sdir"][:H + G].astype(np.float64) - dl)
    dbound = 2 * U + np.concatenate([np.zeros((H, 3)), 6 * U * mag[H:] * 2]) / far
    assert (derr <= dbound).all(), float(derr.max())
    perr = np.abs(r["spos"][:H + G].astype(np.float64) - (start + dl * f32(0.1)))
    pbound = np.concatenate([3 * U * (mag[:H] + 0.1), 6 * U * (mag[H:] + 0.1)])
    assert (perr <= pbound).all(), float(perr.max())
    seg = np.concatenate([hit_off, H + gnd_off[1:]])
    assert np.array_equal(r["sseg"], seg)
    assert np.array_equal(r["scounts"][:2 * S], np.diff(seg)) and not r["scounts"][2 * S:].any()
    assert np.array_equal(r["sactive"][:H + G], np.arange(H + G))
    r.update(fragile=int(fragile.sum()), dir_err=float(derr.max()) if derr.size else 0.0, pos_err=float(perr.max()) if perr.size else 0.0,
             dirs=dirs, nh=nh)
    return r


def shade_reference(slot, hit_pos, grad, shadow, dirs, M, S, H, light, color):
    """(uint8 image [S*M,3] by truncation, mask of channels whose 255 * value is within 1e-3 of an integer)."""
    pix = np.arange(S * M) % M
    value = np.ones((S * M, 3))
    k = np.flatnonzero(slot >= 0)
    h = slot[k]
    g = grad[h].astype(np.float32)
    gn = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    nf = g / gn[:, None]                                   # normalised in float32
    d = dirs[pix[k]].astype(np.float32)
    seen = 1.0 - shadow[h].astype(np.float64)
    ld = light[None, :] - hit_pos[h].astype(np.float64)
    ld /= np.linalg.norm(ld, axis=1, keepdims=True)
    n64, d64 = nf.astype(np.float64), d.astype(np.float64)
    dn = (ld * n64).sum(axis=1)
    diffuse = np.clip(dn, 0, 1) * seen
    refl = ld - 2 * dn[:, None] * n64
    refl /= np.linalg.norm(refl, axis=1, keepdims=True)
    spec = np.clip((refl * d64).sum(axis=1), 0, 1) ** 20 * seen
    rim = -(nf[:, 0] * d[:, 0] + nf[:, 1] * d[:, 1] + nf[:, 2] * d[:, 2])          # float32
    rim = np.float32(1) - np.clip(rim, np.float32(0), np.float32(1))
    rim = rim * rim * rim * rim * np.float32(0.3)
    value[k] = np.clip(color[None, :] * (diffuse * 0.5 + 0.5)[:, None] + (spec * 0.3 + rim.astype(np.float64))[:, None], 0, 1)
    gk = np.flatnonzero(slot <= -2)
    value[gk] -= (np.float32(0.35) * shadow[H + (-2 - slot[gk])].astype(np.float32)).astype(np.float64)[:, None]
    scaled = value * 255.0
    near = np.abs(scaled - np.round(scaled)) < 1e-3
    kind = np.where(slot >= 0, 0, np.where(slot <= -2, 1, 2))
    return np.floor(scaled).astype(np.uint8), near, kind


def check_shade(dev, scene, M, S, seed=4):
    rng = np.random.RandomState(seed)
    H, G = scene["H"], scene["G"]
    grad = rng.normal(size=(max(H, 1), 3))
    grad *= np.exp(rng.uniform(-9, 9, size=(max(H, 1), 1))) / np.linalg.norm(grad, axis=1, keepdims=True)
    grad = grad.astype(np.float32)
    assert (np.abs(grad).max(axis=1) > 0).all()
    shadow = (rng.uniform(size=max(H + G, 1)) < 0.5).astype(np.uint8)
    color = np.array([0.8, 0.1, 0.1])
    t = scene["tensors"]
    image = torch.full((S * M, 3), 77, dtype=torch.uint8, device=dev)
    grad_t, shadow_t = torch.from_numpy(grad).to(dev), torch.from_numpy(shadow).to(dev)
    check(ops._lib().sg_raymarch_shade(ptr(t["slot"]), ptr(t["hit_pos"]), ptr(grad_t), ptr(shadow_t), ptr(t["dirs"]), M, S, H,
                                       doubles(scene["light"]),
                                       doubles(color), ptr(image), stream()), "raymarch_shade")
    got = npy(image).astype(np.int64)
    ref, near, kind = shade_reference(scene["slot"].astype(np.int64), scene["hit_pos"], grad, shadow, scene["dirs"], M, S, H,
                                      scene["light"], color)
    ref = ref.astype(np.int64)
    assert np.array_equal(got[kind == 2], np.full_like(got[kind == 2], 255)), "white pixels"
    assert np.array_equal(got[kind == 1], ref[kind == 1]), "ground pixels"
    assert set(np.unique(ref[kind == 1])) <= {255, 165}
    diff = np.abs(got - ref)
    assert (diff[~near] == 0).all(), int((diff[~near] != 0).sum())
    assert (diff <= 1).all()
    return dict(channels=int((kind == 0).sum()) * 3, near_integer=int(near[kind == 0].sum()), different=int((diff != 0).sum()))


# ------------------------------------------------------------------------------------------------------------------------
# marching cubes (sg_mc_count / sg_mc_emit)
# ------------------------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", os.path.join(HERE, "..", "scripts", "gen_mc_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


_TABLE = []


def case_table():
    """Triangles (edge triples) of the 256 cases from scripts/gen_mc_tables.py's generator (not from csrc/mc_tables.h)."""
    if not _TABLE:
        gen = _generator()
        flip = gen.orientation_flip()
        _TABLE.append([gen.case_triangles(c, flip) for c in range(256)])
    return _TABLE[0]


def check_case_table_orientation():
    """In the unit cube with mid-edge vertices, (v1 - v0) x (v2 - v0) of every triangle of every case points from the inside
    corners of its three edges toward their outside corners: toward increasing values."""
    gen = _generator()
    for case, tris in enumerate(case_table()):
        for tri in tris:
            m = [gen.edge_mid(e) for e in tri]
            n = np.cross(m[1] - m[0], m[2] - m[0])
            out = np.zeros(3)
            for e in tri:
                a, b = gen.edge_corners(e)
                assert ((case >> a) & 1) != ((case >> b) & 1), (case, e)
                i, o = (a, b) if (case >> a) & 1 else (b, a)
                out += gen.corner_pos(o) - gen.corner_pos(i)
            assert np.dot(n, out) > 0, (case, tri)


def _gradient(padded, k, spacing):
    if padded.shape[k] < 2:
        return np.zeros_like(padded)       # a single layer has no difference along k
    return np.gradient(padded, axis=k, edge_order=1) / spacing


def mc_reference(grid, level, pad, pad_value, spacing, origin):
    """One grid [R0,R1,R2] (float32).  dict(pos [V,3], normal [V,3], nbound [V], faces [F,3]) in float64 / int64, in the
    order of the header: vertices by owning corner (row-major), then axis; triangles by cell (row-major), then table order."""
    level, pad_value = f32(level), f32(pad_value)
    sp = np.array([f32(v) for v in spacing])
    org = np.array([f32(v) for v in origin])
    g = grid.astype(np.float64)
    if pad:
        g = np.pad(g, 1, constant_values=pad_value)
    P = g.shape
    inside = g < level
    cross = np.zeros(P + (3,), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    a, b, c, k = np.nonzero(cross)                    # row-major corners, then the axis: the order of the contract
    idx = np.stack([a, b, c], axis=1)
    nxt = idx.copy()
    nxt[np.arange(len(k)), k] += 1
    va, vb = g[tuple(idx.T)], g[tuple(nxt.T)]
    t = (level - va) / (vb - va)
    shift = np.zeros((len(k), 3))
    shift[np.arange(len(k)), k] = t
    pos = (idx + shift) * sp + org
    grads = [_gradient(g, j, sp[j]) for j in range(3)]
    g0 = np.stack([grads[j][tuple(idx.T)] for j in range(3)], axis=1)
    g1 = np.stack([grads[j][tuple(nxt.T)] for j in range(3)], axis=1)
    n = g0 + t[:, None] * (g1 - g0)
    length = np.linalg.norm(n, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        normal = np.where(length[:, None] > 0, n / length[:, None], 0.0)
        # conditioning: each float32 gradient carries 3 roundings (subtract, the spacing product, divide), the interpolation
        # g0 + t (g1 - g0) with a t of 3 roundings adds the rest: at most 22 U of the largest gradient term G per component,
        # sqrt(3) times that for the vector, divided by the un-normalised length; 3 U for the square root and the division
        G = np.maximum(np.abs(g0), np.abs(g1)).max(axis=1)
        nbound = np.where(length > 0, 22 * math.sqrt(3) * U * G / length + 3 * U, np.inf)
    vid = np.full(P + (3,), -1, dtype=np.int64)
    vid[a, b, c, k] = np.arange(len(k))
    # cells
    table = case_table()
    faces = np.zeros((0, 3), dtype=np.int64)
    if min(P) >= 2:
        case = np.zeros(tuple(p - 1 for p in P), dtype=np.int64)
        for corner in range(8):
            o = ((corner >> 2) & 1, (corner >> 1) & 1, corner & 1)
            case |= inside[o[0]:P[0] - 1 + o[0], o[1]:P[1] - 1 + o[1], o[2]:P[2] - 1 + o[2]].astype(np.int64) << corner
        flat = case.reshape(-1)
        ntri = np.array([len(t) for t in table], dtype=np.int64)[flat]
        first = np.concatenate([[0], np.cumsum(ntri)])          # triangles by cell (row-major), then in table order
        faces = np.full((int(first[-1]), 3), -1, dtype=np.int64)
        ca, cb, cc = np.unravel_index(np.arange(flat.size), case.shape)
        for cs in np.unique(flat):
            sel = np.flatnonzero(flat == cs)
            for j, tri in enumerate(table[cs]):
                for kk, e in enumerate(tri):
                    axis, u, w = e >> 2, (e >> 1) & 1, e & 1
                    o = [0, 0, 0]
                    others = [x for x in range(3) if x != axis]
                    o[others[0]], o[others[1]] = u, w
                    faces[first[sel] + j, kk] = vid[ca[sel] + o[0], cb[sel] + o[1], cc[sel] + o[2], axis]
    assert (faces >= 0).all()
    return dict(pos=pos, normal=normal, nbound=nbound, faces=faces)


def noise_grid(shape, seed, level, exact=False):
    g = torch.rand(tuple(shape), generator=torch.Generator().manual_seed(seed)) * 2 - 1
    if exact:       # some corners exactly at the level (they are outside: v < level is false; t is 0 or 1 there)
        mask = torch.rand(tuple(shape), generator=torch.Generator().manual_seed(seed + 1000)) < 0.15
        g[mask] = float(np.float32(level))
    return g


def mc_batch(shape, level, pad_value, seed, S=3):
    """Noise, a blank grid (constant pad_value: no crossing anywhere) in the middle, noise with values exactly at the level, ..."""
    grids = []
    for s in range(S):
        if s % 3 == 1:
            grids.append(torch.full(tuple(shape), float(pad_value)))
        else:
            grids.append(noise_grid(shape, seed + s, level, exact=(s % 3 == 2)))
    return torch.stack(grids)


MC_SHAPES = [(6, 5, 7), (1, 9, 4), (17, 3, 31), (2, 2, 2), (1, 1, 1), (16, 16, 17), (33, 32, 31)]
MC_LEVELS = [(0.0, 1.0), (0.13, 0.4), (-0.2, -1.0)]
MC_SPACING = (0.11, 0.07, 0.05)
MC_ORIGIN = (0.5, -0.5, 0.25)


def closed_and_oriented(faces):
    """Every directed edge occurs once and its reverse once."""
    if len(faces) == 0:
        return True
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    key = e[:, 0] * (faces.max() + 1) + e[:, 1]
    rev = e[:, 1] * (faces.max() + 1) + e[:, 0]
    return len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rev))


def check_mc(batch, grids, level, pad, pad_value, spacing=MC_SPACING, origin=MC_ORIGIN):
    """batch: the MeshBatch of marching_cubes(grids, ...).  Returns dict(pos_err, pos_bound, normal_err, normal_ratio, verts, tris)."""
    vo, to = npy(batch.vert_offsets), npy(batch.tri_offsets)
    V, Nn, Fc = npy(batch.vertices).astype(np.float64), npy(batch.normals).astype(np.float64), npy(batch.faces)
    assert vo[0] == 0 and to[0] == 0 and vo[-1] == V.shape[0] and to[-1] == Fc.shape[0]
    assert np.isfinite(V).all() and np.isfinite(Nn).all()
    out = dict(pos_err=0.0, pos_bound=0.0, normal_err=0.0, normal_ratio=0.0, verts=int(vo[-1]), tris=int(to[-1]))
    for s in range(grids.shape[0]):
        ref = mc_reference(npy(grids[s]), level, pad, pad_value, spacing, origin)
        assert vo[s + 1] - vo[s] == len(ref["pos"]), ("vertex count", s)
        assert to[s + 1] - to[s] == len(ref["faces"]), ("triangle count", s)
        f = Fc[to[s]:to[s + 1]]
        assert np.array_equal(f, ref["faces"]), ("faces", s)
        if len(ref["pos"]) == 0:
            continue
        assert f.size == 0 or (f.min() >= 0 and f.max() < len(ref["pos"]))
        if pad:
            assert closed_and_oriented(f), s
        v, n = V[vo[s]:vo[s + 1]], Nn[vo[s]:vo[s + 1]]
        pb = 2 * float(ulp32(np.abs(ref["pos"]).max()))
        pe = float(np.abs(v - ref["pos"]).max())
        assert pe <= pb, ("position", s, pe, pb)
        ne = np.abs(n - ref["normal"]).max(axis=1)
        assert (ne <= ref["nbound"]).all(), ("normal", s, float((ne / ref["nbound"]).max()))
        out["pos_err"], out["pos_bound"] = max(out["pos_err"], pe), max(out["pos_bound"], pb)
        out["normal_err"] = max(out["normal_err"], float(ne.max()))
        out["normal_ratio"] = max(out["normal_ratio"], float((ne / ref["nbound"]).max()))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# surface sampling (sg_mesh_sample)
# ------------------------------------------------------------------------------------------------------------------------
def special_uniforms(u):
    """Plants the edge cases in the first samples of every shape (as many as fit): u0 = 0, u0 = 1 - 2^-24, u1 + u2 = 1 exactly,
    u1 = u2 = 0."""
    special = torch.tensor([[0.0, 0.3, 0.4], [1.0 - 2.0 ** -24, 0.6, 0.7], [0.5, 0.25, 0.75], [0.37, 0.0, 0.0]])
    S, P = u.shape[0], u.shape[1]
    for s in range(S):
        for j in range(min(P, 4)):
            u[s, j] = special[(s + j) % 4]
    return u


def check_sampling(vertices, faces, vert_offsets, tri_offsets, uniforms, points, empty):
    """All arguments numpy.  Returns dict(samples, fragile, err_ratio)."""
    S, P = uniforms.shape[0], uniforms.shape[1]
    u = uniforms.astype(np.float32)
    samples = fragile_total = 0
    worst = 0.0
    for s in range(S):
        f = faces[tri_offsets[s]:tri_offsets[s + 1]]
        assert empty[s] == (1 if len(f) == 0 else 0)
        if len(f) == 0:
            assert not points[s].any()
            continue
        v = vertices[vert_offsets[s]:vert_offsets[s + 1]].astype(np.float64)
        v0, e1, e2 = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        cdf = np.cumsum(np.linalg.norm(np.cross(e1, e2), axis=1))
        total = cdf[-1]
        x = u[s, :, 0].astype(np.float64) * total
        k = np.minimum(np.searchsorted(cdf, x, side="left"), len(f) - 1)
        tol = 1e-12 * total
        k_lo = np.minimum(np.searchsorted(cdf, x - tol, side="left"), len(f) - 1)
        k_hi = np.minimum(np.searchsorted(cdf, x + tol, side="right"), len(f) - 1)
        near = np.searchsorted(cdf, x - tol, side="left") != np.searchsorted(cdf, x + tol, side="right")
        u1, u2 = u[s, :, 1], u[s, :, 2]
        flip = (u1 + u2) > np.float32(1)                       # float32, as the kernel receives them
        p = np.where(flip, 1.0 - u1.astype(np.float64), u1.astype(np.float64))
        r = np.where(flip, 1.0 - u2.astype(np.float64), u2.astype(np.float64))
        got = points[s].astype(np.float64)

        def at(kk):
            ref = v0[kk] + (p[:, None] * e1[kk] + r[:, None] * e2[kk])
            # eight float32 roundings (1 - u, two edge differences, two products, two sums and the inputs' own), each at most U
            # of a term no larger than |v0| + |e1| + |e2| + |result|
            bound = 8 * U * (np.abs(v0[kk]) + np.abs(e1[kk]) + np.abs(e2[kk]) + np.abs(ref))
            return np.abs(got - ref), bound

        err, bound = at(k)
        good = (err <= bound).all(axis=1)
        for kk in (k_lo, k_hi):       # a fragile sample may take the triangle on the other side of the boundary
            e2_, b2_ = at(kk)
            good |= near & (e2_ <= b2_).all(axis=1)
        assert good.all(), ("sample", s, int((~good).sum()), float((err / np.maximum(bound, 1e-300)).max()))
        sure = ~near
        if sure.any():
            worst = max(worst, float((err[sure] / np.maximum(bound[sure], 1e-300)).max()))
        samples += P
        fragile_total += int(near.sum())
    return dict(samples=samples, fragile=fragile_total, err_ratio=worst)


def hand_mesh():
    """Three packed shapes: a tetrahedron with a zero-area triangle in the middle of its faces, an empty shape, a quad."""
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0],
                      [2, 2, 2], [3, 2, 2], [3, 3.5, 2], [2, 3.5, 2.25]], dtype=torch.float32)
    f = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 4, 2], [1, 2, 3], [0, 3, 2],      # [1, 4, 2]: three collinear points
                      [0, 1, 2], [0, 2, 3]], dtype=torch.int64)
    return v, f, torch.tensor([0, 5, 5, 9], dtype=torch.int64), torch.tensor([0, 5, 5, 7], dtype=torch.int64)
