"""The latent-space traversal animation: a t-SNE map of all latent codes, a stop per cluster, a round trip through the stops, a periodic
spline through their codes, and per frame the mesh of the code next to the map.

The reference's demo_latent_space.py does this with scikit-learn (TSNE, KMeans), scipy (CubicSpline), one get_mesh + MeshRenderer image
and one matplotlib savefig per frame ("about 40 minutes" in its README), and cannot run as published: it raises NotImplementedError
('A labels tensor needs to be supplied here.') before the embedding.  Here labels are optional, and

    tsne             exact t-SNE on the kernels of csrc/tsne.hip (K17): every iteration is queued without a synchronisation
    kmeans           k-means++ and Lloyd in float64 (torch; not a hot path)
    choose_stops     per cluster the point nearest its centre (demo_latent_space.py:64-72)
    round_trip       nearest neighbour, then 2-opt to a local optimum: deterministic, where the reference tries random swaps
    periodic_spline  scipy.interpolate.CubicSpline(..., bc_type='periodic') at integer knots
    traversal_frames SDFNet.voxel_grids -> mesh.marching_cubes -> MeshRenderer.render_meshes, a chunk of frames per pass
    map_panel        the map without matplotlib: discs and the path through evaluation.nearest_neighbours on pixel centres

CPU tensors run on the C++ twin, CUDA tensors on the HIP kernels (shapegan_amd/lib.py).

    python -m shapegan_amd.traversal --net models/sdf_net.to --codes models/sdf_net_latent_codes.to --out images/ [--labels labels.to]
        [--stops 30] [--transition-frames 60] [--resolution 128] [--size 1080] [--device cuda|cpu] [--embedding-out emb.to] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np
import torch

from . import lib as L
from . import mesh as M
from .brickgrid import options as narrow_band_options
from .topology import clean_option
from . import ops

SURFACE_LEVEL = 0.011      # demo_latent_space.py:19
PALETTE = ((0.122, 0.467, 0.706), (1.000, 0.498, 0.055), (0.173, 0.627, 0.173), (0.839, 0.153, 0.157), (0.580, 0.404, 0.741),
           (0.549, 0.337, 0.294), (0.890, 0.467, 0.761), (0.498, 0.498, 0.498), (0.737, 0.741, 0.133), (0.090, 0.745, 0.812))
ONE_COLOR = PALETTE[0]
PATH_COLOR = (0.2, 0.2, 0.2)
EDGE_COLOR = (0.1, 0.1, 0.1)


# ---- the embedding --------------------------------------------------------------------------------------------------------------------
def pca_init(codes):
    """[N, 2] float64: the first two principal components of the codes (float64 SVD of the centred table), scaled so that the first
    has standard deviation 1e-4 (scikit-learn's init="pca").  Sign: each component is oriented so that its loading of largest
    magnitude is positive.  A table with one column has no second component: that coordinate starts at zero."""
    x = codes.detach().double().cpu()
    x = x - x.mean(dim=0, keepdim=True)
    _, _, vt = torch.linalg.svd(x, full_matrices=False)
    vt = vt[:2]
    big = vt.abs().argmax(dim=1)
    vt = vt * torch.sign(vt[torch.arange(vt.shape[0]), big]).unsqueeze(1)
    y = x @ vt.t()
    if y.shape[1] < 2:
        y = torch.cat([y, torch.zeros(y.shape[0], 2 - y.shape[1], dtype=torch.float64)], dim=1)
    return y / y[:, 0].std(unbiased=False) * 1e-4


def auto_learning_rate(n, exaggeration):
    return max(n / float(exaggeration) / 4.0, 50.0)


def tsne(codes, perplexity=30, iterations=1000, exaggeration=12, exaggeration_iterations=250, lr="auto", init="pca", seed=0,
         return_kl=False):
    """The exact t-SNE embedding [N, 2] (float32, on the device of `codes`) of codes [N, D]; with return_kl also the final KL
    divergence (a float).

    scikit-learn's TSNE(method="exact") with its defaults: early exaggeration `exaggeration` with momentum 0.5 for the first
    `exaggeration_iterations` iterations, momentum 0.8 afterwards, gains as in _gradient_descent, lr="auto" = max(N / exaggeration / 4,
    50).  init: "pca" (pca_init), "random" (a normal draw from torch.Generator().manual_seed(seed), times 1e-4) or an explicit [N, 2]
    tensor.  The iteration count is FIXED: scikit-learn's early stop (no progress for 300 iterations, gradient norm below 1e-7) is left
    out, so that the loop never reads anything back and all iterations are queued at once."""
    if not torch.is_tensor(codes):
        codes = torch.as_tensor(np.asarray(codes))
    if codes.dim() != 2:
        raise ValueError("tsne: codes must be [N, D], got %s" % (tuple(codes.shape),))
    dev, N = codes.device, codes.shape[0]
    if torch.is_tensor(init):
        if tuple(init.shape) != (N, 2):
            raise ValueError("tsne: init must be [%d, 2], got %s" % (N, tuple(init.shape)))
        y0 = init.detach()
    elif init == "pca":
        y0 = pca_init(codes)
    elif init == "random":
        y0 = torch.randn((N, 2), generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32) * 1e-4
    else:
        raise ValueError("tsne: init must be 'pca', 'random' or a tensor, got %r" % (init,))
    if lr == "auto":
        lr = auto_learning_rate(N, exaggeration)
    y = y0.to(device=dev, dtype=torch.float32).contiguous().clone()
    P, _, plogp = ops.tsne_affinities(codes, perplexity)
    velocity, gains = torch.zeros_like(y), torch.ones_like(y)
    grad = torch.empty_like(y)
    for it in range(int(iterations)):
        early = it < int(exaggeration_iterations)
        ops.tsne_step(y, P, velocity, gains, exaggeration if early else 1.0, 0.5 if early else 0.8, lr, grad=grad)
    if not return_kl:
        return y
    _, kl = ops.tsne_gradient(y, P, 1.0, plogp)
    return y, float(kl.item())


# ---- stops and the tour ---------------------------------------------------------------------------------------------------------------
def kmeans(points, k, seed=0, max_iterations=300):
    """(centres [k, C] float64, assignment [N] int64) of points [N, C]: k-means++ seeding from torch.Generator().manual_seed(seed),
    then Lloyd's iteration in float64 until the assignment stops changing (or max_iterations).  An emptied cluster keeps its centre."""
    x = torch.as_tensor(np.asarray(points) if not torch.is_tensor(points) else points).detach().double().cpu()
    n, k = x.shape[0], int(k)
    if not 1 <= k <= n:
        raise ValueError("kmeans: k = %d for %d points" % (k, n))
    g = torch.Generator().manual_seed(int(seed))
    centres = [x[int(torch.randint(n, (1,), generator=g))]]
    d2 = ((x - centres[0]) ** 2).sum(dim=1)
    for _ in range(1, k):
        total = float(d2.sum())
        pick = int(torch.multinomial(d2 / total, 1, generator=g)) if total > 0 else int(torch.randint(n, (1,), generator=g))
        centres.append(x[pick])
        d2 = torch.minimum(d2, ((x - centres[-1]) ** 2).sum(dim=1))
    centres = torch.stack(centres)
    assign = None
    for _ in range(int(max_iterations)):
        new = torch.cdist(x, centres).argmin(dim=1)
        if assign is not None and torch.equal(new, assign):
            break
        assign = new
        for c in range(k):
            members = x[assign == c]
            if members.shape[0]:
                centres[c] = members.mean(dim=0)
    return centres, assign


def choose_stops(embedding, k, labels=None, seed=0):
    """Indices [k] (int64) of one stop per k-means cluster of the embedding: the point nearest the cluster's centre; with labels, the
    nearest among the points that carry the cluster's majority label (demo_latent_space.py:64-72)."""
    x = torch.as_tensor(np.asarray(embedding) if not torch.is_tensor(embedding) else embedding).detach().double().cpu()
    centres, assign = kmeans(x, k, seed=seed)
    if labels is not None:
        labels = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).detach().cpu().long()
    stops = []
    for c in range(int(k)):
        dist = (x - centres[c]).norm(dim=1)
        if labels is not None and bool((assign == c).any()):
            majority = int(torch.bincount(labels[assign == c]).argmax())
            dist = torch.where(labels == majority, dist, torch.full_like(dist, float("inf")))
        stops.append(int(dist.argmin()))
    return torch.tensor(stops, dtype=torch.int64)


def _tour_length(d, order):
    return float(d[order, np.roll(order, -1)].sum())


def two_opt_move(d, order):
    """The first (i, j), in scan order, whose reversal of order[i + 1 .. j] would shorten the closed tour under the distance matrix d,
    or None."""
    K = len(order)
    for i in range(K - 1):
        for j in range(i + 2, K if i > 0 else K - 1):
            a, b, c, e = order[i], order[i + 1], order[j], order[(j + 1) % K]
            if d[a, c] + d[b, e] < d[a, b] + d[c, e] - 1e-12 * (1.0 + d[a, b] + d[c, e]):
                return i, j
    return None


def _two_opt(d, order):
    order = np.array(order, dtype=np.int64)
    while True:
        move = two_opt_move(d, order)
        if move is None:
            return order
        i, j = move
        order[i + 1:j + 1] = order[i + 1:j + 1][::-1].copy()


def round_trip(points):
    """A short closed tour through points [K, C]: the order [K] (int64, a permutation).  Two starts — nearest neighbour from point 0
    (the lowest index of a tie) and the input order — are each improved by 2-opt (reversing a stretch of the tour whenever that
    shortens it, scanning in a fixed order) until no move does; the shorter result is returned, the first on a tie.  Deterministic,
    2-opt optimal and never longer than the input order.  The reference (demo_latent_space.py:74-98) tries 500 000 random swaps."""
    x = torch.as_tensor(np.asarray(points) if not torch.is_tensor(points) else points).detach().double().cpu().numpy()
    K = x.shape[0]
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    order, left = [0], set(range(1, K))
    while left:
        here = order[-1]
        nxt = min(left, key=lambda j: (d[here, j], j))
        order.append(nxt)
        left.remove(nxt)
    best = _two_opt(d, order)
    other = _two_opt(d, np.arange(K))
    if _tour_length(d, other) < _tour_length(d, best):
        best = other
    return torch.from_numpy(best)


def periodic_spline(values, t):
    """The periodic cubic spline through values [K + 1, C] (last row equal to the first) at the knots 0 .. K, evaluated at t [T]:
    [T, C] float64 — scipy.interpolate.CubicSpline(np.arange(K + 1), values, axis=0, bc_type='periodic')(t).  The second derivatives
    m_i solve the cyclic tridiagonal system m_{i-1} + 4 m_i + m_{i+1} = 6 (v_{i-1} - 2 v_i + v_{i+1}) in float64; any t is taken
    modulo K."""
    v = torch.as_tensor(np.asarray(values) if not torch.is_tensor(values) else values).detach().double().cpu()
    t = torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).detach().double().cpu().reshape(-1)
    if v.dim() != 2 or v.shape[0] < 2:
        raise ValueError("periodic_spline: values must be [K + 1, C] with K >= 1, got %s" % (tuple(v.shape),))
    if not torch.equal(v[0], v[-1]):
        raise ValueError("periodic_spline: the last row must equal the first")
    K = v.shape[0] - 1
    y = v[:K]
    A = torch.zeros((K, K), dtype=torch.float64)
    idx = torch.arange(K)
    A[idx, idx] += 4.0
    A[idx, (idx + 1) % K] += 1.0
    A[idx, (idx - 1) % K] += 1.0
    rhs = 6.0 * (y[(idx - 1) % K] - 2.0 * y + y[(idx + 1) % K])
    m = torch.linalg.solve(A, rhs)
    tm = torch.remainder(t, float(K))
    i = torch.clamp(torch.floor(tm).long(), 0, K - 1)
    u = (tm - i.double()).unsqueeze(1)
    w = 1.0 - u
    j = (i + 1) % K
    return y[i] * w + y[j] * u + ((w * w * w - w) * m[i] + (u * u * u - u) * m[j]) / 6.0


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
def _frame_bytes(voxel_resolution, size, ssaa):
    """A generous bound on what one frame of a chunk holds on the device at a time: the sample grid with its MLP activations' worth of
    scratch, the padded grid, and the supersampled picture with depth and colour."""
    R, n = int(voxel_resolution), int(size) * int(ssaa)
    return 16 * (R + 2) ** 3 * 4 + n * n * 24


def traversal_frames(sdf_net, frame_codes, voxel_resolution=128, level=SURFACE_LEVEL, size=1080, chunk=None, model_color=None,
                     renderer=None, memory_budget=2 << 30, narrow_band=False, refine=0, clean=False):
    """Generator of uint8 [size, size, 3] images, one per row of frame_codes [F, L]: frame f is
        viewer.set_mesh(sdf_net.get_mesh(frame_codes[f], voxel_resolution, level=level)); viewer.get_image()
    of a fresh MeshRenderer(size=size), byte for byte, but a chunk of frames goes through voxel_grids -> marching_cubes -> render_meshes
    together.  chunk: frames per pass (default: what memory_budget bytes hold, at most mesh.max_shapes_per_call).  One model_color for
    the whole call (a colour per frame would need a colour per shape in the raster shading kernel).  A code whose grid does not cross
    `level` yields floor and background.  renderer: a MeshRenderer to use (its size wins).  narrow_band: the grids come from the brick
    path of SDFNet.voxel_grids, built for `level` (True, or a dict of its arguments brick / band / lipschitz; the same frames, byte for byte, whenever the meshes are the same).
    refine = K > 0: every frame's mesh is get_mesh(..., refine=K) — vertices on the network's level set, its normals (surface.refine_meshes).
    clean: a rule of topology.clean_meshes ("largest", True, a dict) applied to every frame's mesh before refine (no flickering floaters)."""
    from .rendering import MeshRenderer
    dev = next(sdf_net.parameters()).device
    codes = frame_codes.detach().reshape(-1, sdf_net.latent_code_size).to(device=dev, dtype=torch.float32)
    viewer = renderer if renderer is not None else MeshRenderer(size=size, start_thread=False)
    if model_color is not None:
        viewer.model_color = tuple(float(c) for c in model_color)
    R = int(voxel_resolution)
    per = min(M.max_shapes_per_call((R, R, R), True), max(1, int(memory_budget) // _frame_bytes(R, viewer.size, viewer.ssaa)))
    per = max(1, min(per, int(chunk))) if chunk else per
    with torch.no_grad():
        for a in range(0, codes.shape[0], per):
            grids = sdf_net.voxel_grids(codes[a:a + per], R, sphere_only=True, level=level, **narrow_band_options(narrow_band))
            batch = M.marching_cubes(grids, level=level, spacing=2.0 / R, origin=-1.0, pad=True, pad_value=1.0)
            if clean:
                batch = batch.clean(clean)
            if refine:
                from .surface import cell_diagonal, refine_meshes
                batch, _ = refine_meshes(sdf_net, codes[a:a + per], batch, level=level, iterations=int(refine), max_move=cell_diagonal(R))
            for image in viewer.render_meshes(batch):
                yield image


# ---- the map --------------------------------------------------------------------------------------------------------------------------
def label_colors(labels, count):
    """[count, 3] float32 in 0..1: PALETTE[label mod 10] per point, ONE_COLOR for all without labels."""
    if labels is None:
        return torch.tensor(ONE_COLOR, dtype=torch.float32).repeat(int(count), 1)
    labels = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).detach().cpu().long()
    return torch.tensor(PALETTE, dtype=torch.float32)[labels % len(PALETTE)]


class MapPanel(object):
    """The map of an embedding as an image: every point a disc in its colour, the path a dark line, the stops larger discs with a dark
    rim — drawn ONCE, by nearest-neighbour queries from the pixel centres (evaluation.nearest_neighbours: a pixel takes the colour of
    its nearest point if that point lies within the disc radius).  image(marker) composes the current frame's marker, in torch.

    Geometry follows demo_latent_space.py:127-155 at its 1080 pixels, scaled with `size`: axes from min - margin to max + margin per
    coordinate, over the points and the path (margin: 5 % of the larger extent), y upwards; scatter sizes 10 / 140 / 200 points^2 and a 2-point line at 100 dpi are
    discs of radius 2.2 / 8.2 / 9.8 pixels and a half-width of 1.4 pixels (never less than 0.75 / 1.5 / 1.5 / 0.75 pixels).  Layers from the bottom: points, path, marker, stops."""

    def __init__(self, embedding, colors, path, stops, size=1080, device=None):
        from . import evaluation
        emb = torch.as_tensor(np.asarray(embedding) if not torch.is_tensor(embedding) else embedding).detach()
        dev = torch.device(device) if device is not None else emb.device
        emb = emb.double().cpu()
        self.size, self.device = int(size), dev
        scale = self.size / 1080.0
        floor = 0.75      # (more than half a pixel's diagonal: the pixel that holds a centre is always inside its disc)
        self.r_point, self.r_stop, self.r_marker = max(2.2 * scale, floor), max(8.2 * scale, 2 * floor), max(9.8 * scale, 2 * floor)
        self.half_line, self.rim = max(1.4 * scale, floor), min(1.4 * scale, floor)
        extent = emb
        if path is not None and len(path) >= 1:      # (a spline overshoots between stops: the axes hold the path as well)
            path = torch.as_tensor(np.asarray(path) if not torch.is_tensor(path) else path).detach().double().cpu().reshape(-1, 2)
            extent = torch.cat([emb, path])
        lo, hi = extent.min(dim=0)[0], extent.max(dim=0)[0]
        margin = 0.05 * float((hi - lo).max()) or 1.0
        self.lo, self.span = lo - margin, (hi - lo) + 2 * margin
        colors = torch.as_tensor(np.asarray(colors) if not torch.is_tensor(colors) else colors).detach().float().cpu()
        if colors.dim() == 1:
            colors = colors.repeat(emb.shape[0], 1)
        self.colors = colors
        n = self.size
        centres = torch.arange(n, dtype=torch.float32, device=dev) + 0.5
        self.pixels = torch.stack([centres.repeat(n), centres.repeat_interleave(n), torch.zeros(n * n, device=dev)], dim=1)   # x fastest

        def nearest(points_px):
            cloud = torch.cat([points_px, torch.zeros(points_px.shape[0], 1, dtype=points_px.dtype)], dim=1).float().to(dev)
            d2, idx, _, _ = evaluation.nearest_neighbours(self.pixels.unsqueeze(0), cloud.unsqueeze(0))
            return d2[0], idx[0].long()

        image = torch.ones((n * n, 3), dtype=torch.float32, device=dev)
        d2, idx = nearest(self.to_pixels(emb))
        inside = d2 <= self.r_point ** 2
        image[inside] = colors.to(dev)[idx[inside]]
        if path is not None and len(path) >= 1:
            d2, _ = nearest(self._dense(self.to_pixels(path)))
            image[d2 <= self.half_line ** 2] = torch.tensor(PATH_COLOR, device=dev)
        self.stop_mask = torch.zeros(n * n, dtype=torch.bool, device=dev)
        if stops is not None and len(stops) >= 1:
            stops = torch.as_tensor(np.asarray(stops) if not torch.is_tensor(stops) else stops).detach().cpu().long()
            d2, idx = nearest(self.to_pixels(emb[stops]))
            self.stop_mask = d2 <= self.r_stop ** 2
            face = self.stop_mask & (d2 <= (self.r_stop - self.rim) ** 2)
            image[self.stop_mask] = torch.tensor(EDGE_COLOR, device=dev)
            image[face] = colors[stops].to(dev)[idx[face]]
        self.static = image

    def to_pixels(self, xy):
        """Embedding coordinates [M, 2] -> pixel coordinates (x to the right, y downwards), float64."""
        xy = torch.as_tensor(np.asarray(xy) if not torch.is_tensor(xy) else xy).detach().double().cpu().reshape(-1, 2)
        f = (xy - self.lo) / self.span
        return torch.stack([f[:, 0] * self.size, (1.0 - f[:, 1]) * self.size], dim=1)

    @staticmethod
    def _dense(px, step=0.5):
        """The polyline through px [M, 2] sampled at most `step` pixels apart."""
        if px.shape[0] < 2:
            return px
        seg = (px[1:] - px[:-1]).norm(dim=1)
        pieces = []
        for a, b, length in zip(px[:-1], px[1:], seg.tolist()):
            m = max(1, int(np.ceil(length / step)))
            w = (torch.arange(m, dtype=torch.float64) / m).unsqueeze(1)
            pieces.append(a * (1 - w) + b * w)
        pieces.append(px[-1:])
        return torch.cat(pieces)

    def image(self, marker=None, marker_color=None):
        """uint8 [size, size, 3] (numpy): the static layers and, when given, the marker at embedding position `marker` [2]."""
        image = self.static
        if marker is not None:
            c = self.to_pixels(marker)[0].float().to(self.device)
            d2 = ((self.pixels[:, :2] - c) ** 2).sum(dim=1)
            ring = (d2 <= self.r_marker ** 2) & ~self.stop_mask
            face = ring & (d2 <= (self.r_marker - self.rim) ** 2)
            image = image.clone()
            image[ring] = torch.tensor(EDGE_COLOR, device=self.device)
            image[face] = torch.tensor(ONE_COLOR if marker_color is None else tuple(float(v) for v in marker_color), device=self.device)
        n = self.size
        return (image * 255.0 + 0.5).clamp(0, 255).to(torch.uint8).view(n, n, 3).cpu().numpy()


def map_panel(embedding, colors, path, stops, marker, size=1080, marker_color=None, device=None):
    """uint8 [size, size, 3]: the map of MapPanel with the marker at `marker` [2] (None: no marker).  For a sequence of frames keep a
    MapPanel and call image() per frame: the static layers are drawn once."""
    return MapPanel(embedding, colors, path, stops, size=size, device=device).image(marker, marker_color)


# ---- the command line -----------------------------------------------------------------------------------------------------------------
FFMPEG_LINE = "ffmpeg -framerate 30 -i %s -c:v libx264 -profile:v high -crf 19 -pix_fmt yuv420p video.mp4"


def plan_traversal(codes, labels=None, stops=30, transition_frames=60, perplexity=30, iterations=1000, seed=0):
    """The host-side plan of the animation from a table of codes [N, L] (on the device the embedding is to run on): a dict with
    embedding [N, 2], stops [K + 1] (the tour, closed), frame_codes [K T, L] and frame_positions [K T, 2] (both float64, CPU)."""
    embedding = tsne(codes, perplexity=perplexity, iterations=iterations, seed=seed).cpu()
    chosen = choose_stops(embedding, stops, labels=labels, seed=seed)
    tour = chosen[round_trip(embedding[chosen])]
    tour = torch.cat([tour, tour[:1]])
    progress = torch.arange(int(stops) * int(transition_frames), dtype=torch.float64) / int(transition_frames)
    table = codes.detach().double().cpu()
    return dict(embedding=embedding, stops=tour, frame_codes=periodic_spline(table[tour], progress),
                frame_positions=periodic_spline(embedding[tour], progress))


def main(argv=None):
    from PIL import Image
    from .model.sdf_net import SDFNet
    ap = argparse.ArgumentParser(description="Render the latent-space traversal animation of a trained SDFNet.")
    ap.add_argument("--net", required=True, help="state_dict of a trained SDFNet (models/sdf_net.to)")
    ap.add_argument("--codes", required=True, help="its latent table [N, L] (models/sdf_net_latent_codes.to)")
    ap.add_argument("--out", required=True, help="directory for frame-%%05d.png")
    ap.add_argument("--labels", default=None, help="an int tensor [N] of class labels (optional)")
    ap.add_argument("--stops", type=int, default=30)
    ap.add_argument("--transition-frames", type=int, default=60)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--size", type=int, default=1080)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--embedding-out", default=None, help="where the embedding [N, 2] is torch.save'd")
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--narrow-band", action="store_true", help="evaluate the network only in bricks near the surface")
    ap.add_argument("--clean", nargs="?", const="default", default=None, choices=("default", "largest"),
                    help="drop floating pieces of every frame's mesh: below 1 %% of the area (default) or all but the largest")
    args = ap.parse_args(argv)

    state = torch.load(args.net, map_location="cpu")
    net = SDFNet(latent_code_size=state["layers1.0.weight"].shape[1] - 3, device=args.device)
    net.load_state_dict(state)
    L.bump_param_epoch()
    codes = torch.load(args.codes, map_location="cpu").detach().float()
    labels = torch.load(args.labels, map_location="cpu") if args.labels else None
    plan = plan_traversal(codes.to(args.device), labels, args.stops, args.transition_frames, args.perplexity, args.iterations, args.seed)
    if args.embedding_out:
        torch.save(plan["embedding"], args.embedding_out)
    os.makedirs(args.out, exist_ok=True)
    panel = MapPanel(plan["embedding"], label_colors(labels, codes.shape[0]), plan["frame_positions"], plan["stops"][:-1], size=args.size,
                     device=args.device)
    frames = traversal_frames(net, plan["frame_codes"], voxel_resolution=args.resolution, size=args.size, narrow_band=args.narrow_band,
                              clean=clean_option(args.clean))
    for f, (image, position) in enumerate(zip(frames, plan["frame_positions"])):
        Image.fromarray(np.concatenate((image, panel.image(position)), axis=1)).save(os.path.join(args.out, "frame-%05d.png" % f))
    print("\nUse this command to create a video:\n")
    print(FFMPEG_LINE % os.path.join(args.out, "frame-%05d.png"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
