"""shapegan_amd/traversal.py without a GPU, through the twin: the spline, the clustering, the stops, the tour, the map panel, the frames
and the command line.  frames_body and cli_body run again on the device in tests/test_gpu_traversal.py."""
import numpy as np
import pytest
import torch

import latent_fit_forms as LF
import tsne_reference as R
from shapegan_amd import traversal as T


def blobs(per=20, k=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    centres = torch.tensor([[0.0, 0.0], [40.0, 0.0], [0.0, 40.0], [40.0, 40.0], [80.0, 20.0]])[:k]
    labels = torch.arange(k).repeat_interleave(per)
    return centres[labels] + torch.randn(k * per, 2, generator=g), labels


def test_periodic_spline_equals_scipy():
    interpolate = pytest.importorskip("scipy.interpolate")
    rng = np.random.RandomState(0)
    for K, C in ((2, 1), (3, 2), (7, 3), (30, 128)):
        v = rng.randn(K + 1, C)
        v[-1] = v[0]
        t = np.concatenate([np.linspace(0, K, 97), np.arange(K + 1), rng.rand(20) * K])
        ref = interpolate.CubicSpline(np.arange(K + 1), v, axis=0, bc_type="periodic")(t)
        got = T.periodic_spline(v, t).numpy()
        assert got.dtype == np.float64 and got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), (K, C, np.abs(got - ref).max())


def test_periodic_spline_is_periodic_and_interpolates_the_knots_exactly():
    rng = np.random.RandomState(1)
    K = 6
    v = rng.randn(K + 1, 4)
    v[-1] = v[0]
    assert np.array_equal(T.periodic_spline(v, np.arange(K + 1)).numpy(), v)
    t = np.arange(0, K * 8) / 8.0      # dyadic: t + K and t - K are exact
    a = T.periodic_spline(v, t)
    assert torch.equal(a, T.periodic_spline(v, t + K)) and torch.equal(a, T.periodic_spline(v, t - 2 * K))
    h = 1e-6      # the first derivative is continuous across the seam
    left = (T.periodic_spline(v, [K]) - T.periodic_spline(v, [K - h])) / h
    right = (T.periodic_spline(v, [h]) - T.periodic_spline(v, [0.0])) / h
    assert float((left - right).abs().max()) < 1e-4
    with pytest.raises(ValueError):
        T.periodic_spline(rng.randn(4, 2), [0.5])


def test_kmeans_recovers_separated_blobs_and_is_seed_deterministic():
    x, labels = blobs(per=25, k=5)
    for seed in (0, 1, 2):
        centres, assign = T.kmeans(x, 5, seed=seed)
        assert centres.dtype == torch.float64 and assign.dtype == torch.int64
        # the same partition as the labels: every cluster is exactly one blob
        assert sorted(sorted(torch.nonzero(assign == c).flatten().tolist()) for c in range(5)) == \
            sorted(sorted(torch.nonzero(labels == c).flatten().tolist()) for c in range(5))
        for c in range(5):
            assert torch.allclose(centres[c], x[assign == c].double().mean(dim=0), atol=1e-12)
        again = T.kmeans(x, 5, seed=seed)
        assert torch.equal(again[0], centres) and torch.equal(again[1], assign)
    with pytest.raises(ValueError):
        T.kmeans(x, 0)


def test_kmeans_keeps_the_centre_of_an_emptied_cluster():
    x = torch.tensor([[0.0, 0.0]] * 5 + [[1.0, 1.0]] * 5)      # two distinct points, three clusters: one must stay empty
    centres, assign = T.kmeans(x, 3, seed=0)
    assert bool(torch.isfinite(centres).all()) and len(set(assign.tolist())) == 2


def test_choose_stops_picks_within_the_majority_label():
    x, labels = blobs(per=20, k=4)
    noisy = labels.clone()
    noisy[::20] = (noisy[::20] + 1) % 4      # one point per blob carries another blob's label
    plain = T.choose_stops(x, 4, seed=0)
    assert sorted(labels[plain].tolist()) == [0, 1, 2, 3]
    stops = T.choose_stops(x, 4, labels=noisy, seed=0)
    assert stops.dtype == torch.int64 and sorted(noisy[stops].tolist()) == [0, 1, 2, 3]
    _, assign = T.kmeans(x, 4, seed=0)
    for s in stops.tolist():
        cluster = assign[s]
        assert int(noisy[s]) == int(torch.bincount(noisy[assign == cluster]).argmax())
    # a label that forces the choice: the nearest point of a cluster is relabelled, so the stop moves to the nearest of the majority
    forced = labels.clone()
    forced[plain[0]] = (forced[plain[0]] + 1) % 4
    moved = T.choose_stops(x, 4, labels=forced, seed=0)
    assert int(moved[0]) != int(plain[0]) and int(forced[moved[0]]) == int(labels[plain[0]])


def test_round_trip_is_two_opt_optimal_and_no_longer_than_the_input():
    for seed, K in ((0, 4), (1, 9), (2, 30)):
        x = torch.randn(K, 2, generator=torch.Generator().manual_seed(seed))
        order = T.round_trip(x)
        assert sorted(order.tolist()) == list(range(K))
        d = torch.cdist(x.double(), x.double()).numpy()
        assert T.two_opt_move(d, order.numpy()) is None
        length = d[order.numpy(), np.roll(order.numpy(), -1)].sum()
        assert length <= d[np.arange(K), np.roll(np.arange(K), -1)].sum() + 1e-12
        for i in range(K - 1):      # checked here as well, from the definition: no reversal shortens the tour
            for j in range(i + 2, K if i > 0 else K - 1):
                o = order.numpy().copy()
                o[i + 1:j + 1] = o[i + 1:j + 1][::-1]
                assert d[o, np.roll(o, -1)].sum() >= length - 1e-9
        assert torch.equal(order, T.round_trip(x))
    assert T.round_trip(torch.zeros(1, 2)).tolist() == [0]


def test_map_panel_draws_points_background_and_a_moving_marker():
    x, labels = blobs(per=6, k=4)
    colors = T.label_colors(labels, len(labels))
    stops = torch.tensor([0, 6, 12, 18])
    path = T.periodic_spline(torch.cat([x[stops], x[stops[:1]]]), np.arange(40) / 10.0)
    panel = T.MapPanel(x, colors, path, stops, size=256)
    image = panel.image()
    assert image.shape == (256, 256, 3) and image.dtype == np.uint8
    px = panel.to_pixels(x).numpy()
    stop_px = px[stops.numpy()]
    path_px = panel.to_pixels(path).numpy()
    tested = 0
    for i in range(len(x)):      # the pixel that holds a point's centre has its colour, unless the path or a stop lies over it
        col, row = int(px[i, 0]), int(px[i, 1])
        centre = np.array([col + 0.5, row + 0.5])
        if np.linalg.norm(stop_px - centre, axis=1).min() <= panel.r_stop + 1 or np.linalg.norm(path_px - centre, axis=1).min() <= 4:
            continue
        if np.linalg.norm(px - centre, axis=1).argmin() != i:
            continue
        assert np.array_equal(image[row, col], (colors[i].numpy() * 255 + 0.5).astype(np.uint8)), i
        tested += 1
    assert tested >= 8
    for s, i in enumerate(stops.tolist()):      # a stop's centre pixel has the stop's colour
        assert np.array_equal(image[int(stop_px[s, 1]), int(stop_px[s, 0])], (colors[i].numpy() * 255 + 0.5).astype(np.uint8))
    everything = np.concatenate([px, panel._dense(panel.to_pixels(path)).numpy()])
    cols, rows = np.meshgrid(np.arange(256) + 0.5, np.arange(256) + 0.5)
    far = np.ones((256, 256), dtype=bool)
    for q in everything:
        far &= (cols - q[0]) ** 2 + (rows - q[1]) ** 2 > (panel.r_stop + 1) ** 2
    assert far.any() and bool((image[far] == 255).all()), "a pixel farther than every radius from everything is not background"
    a, b = panel.image(path[5]), panel.image(path[25])      # (half way between two stops: a stop is drawn over the marker)
    assert not np.array_equal(a, b) and not np.array_equal(a, image)
    ca = panel.to_pixels(path[5])[0].numpy()
    assert np.array_equal(a[int(ca[1]), int(ca[0])], (np.array(T.ONE_COLOR) * 255 + 0.5).astype(np.uint8))
    assert np.array_equal(panel.image(), image), "composing a marker changed the static layers"
    assert np.array_equal(T.map_panel(x, colors, path, stops, path[5], size=256), a)
    one = T.map_panel(x, T.ONE_COLOR, None, None, None, size=64)
    assert set(map(tuple, one.reshape(-1, 3).tolist())) == {(255, 255, 255), tuple(int(c * 255 + 0.5) for c in T.ONE_COLOR)}


def frames_body(dev):
    """traversal_frames at resolution 16, size 32 on the chairs weights equals the set_mesh + get_image loop byte for byte; a code whose
    grid never crosses the level still yields a frame (floor and background: what a viewer without a mesh shows)."""
    from shapegan_amd.rendering import MeshRenderer
    net = LF.net_on(dev, 5, 128, LF.chairs_state())
    codes = torch.cat([torch.randn(3, 128, generator=torch.Generator().manual_seed(3)) * 0.1, torch.full((1, 128), 50.0),
                       torch.zeros(1, 128)]).to(dev)
    assert net.get_mesh(codes[3], 16, level=T.SURFACE_LEVEL) is None, "the case without a surface has one"
    for chunk in (None, 2):
        frames = list(T.traversal_frames(net, codes, voxel_resolution=16, size=32, chunk=chunk))
        assert len(frames) == 5
        for f, image in enumerate(frames):
            viewer = MeshRenderer(size=32, start_thread=False)
            viewer.set_mesh(net.get_mesh(codes[f], voxel_resolution=16, level=T.SURFACE_LEVEL))
            expected = viewer.get_image()
            assert image.dtype == np.uint8 and image.shape == (32, 32, 3)
            assert np.array_equal(image, expected), "frame %d (chunk %s) differs from set_mesh + get_image" % (f, chunk)
    assert not np.array_equal(frames[0], frames[3])
    blue = list(T.traversal_frames(net, codes[:1], voxel_resolution=16, size=32, model_color=(0.1, 0.1, 0.9)))[0]
    assert not np.array_equal(blue, frames[0])


def cli_body(dev, tmp_path, capsys):
    """12 seeded codes, 4 stops x 3 frames at resolution 16, size 32: 12 PNGs of mesh and map side by side, and an embedding file."""
    from PIL import Image
    torch.save(LF.chairs_state(), str(tmp_path / "sdf_net.to"))
    codes = torch.from_numpy(R.clusters(12, 128, 4, 5)) * 0.05
    torch.save(codes, str(tmp_path / "codes.to"))
    torch.save(torch.arange(12) % 4, str(tmp_path / "labels.to"))
    out = tmp_path / "images"
    rc = T.main(["--net", str(tmp_path / "sdf_net.to"), "--codes", str(tmp_path / "codes.to"), "--labels", str(tmp_path / "labels.to"),
                 "--out", str(out), "--stops", "4", "--transition-frames", "3", "--resolution", "16", "--size", "32", "--device", dev,
                 "--embedding-out", str(tmp_path / "emb.to"), "--perplexity", "3", "--iterations", "50", "--seed", "0"])
    assert rc == 0
    files = sorted(p.name for p in out.iterdir())
    assert files == ["frame-%05d.png" % f for f in range(12)]
    images = [np.asarray(Image.open(str(out / f))) for f in files]
    assert all(im.shape == (32, 64, 3) and im.dtype == np.uint8 for im in images)
    assert any(not np.array_equal(images[0][:, 32:], im[:, 32:]) for im in images[1:]), "the marker never moves"
    emb = torch.load(str(tmp_path / "emb.to"))
    assert emb.shape == (12, 2) and emb.dtype == torch.float32 and bool(torch.isfinite(emb).all())
    text = capsys.readouterr().out
    assert "ffmpeg -framerate 30 -i" in text and "frame-%05d.png" in text


def test_traversal_frames_equal_the_viewer_loop():
    frames_body("cpu")


def test_command_line(tmp_path, capsys):
    cli_body("cpu", tmp_path, capsys)


def test_plan_traversal_closes_the_tour():
    codes = torch.from_numpy(R.clusters(40, 8, 4, 1))
    plan = T.plan_traversal(codes, stops=4, transition_frames=5, perplexity=5, iterations=60)
    assert plan["stops"].shape == (5,) and int(plan["stops"][0]) == int(plan["stops"][-1]) and len(set(plan["stops"].tolist())) == 4
    assert plan["frame_codes"].shape == (20, 8) and plan["frame_positions"].shape == (20, 2)
    assert torch.equal(plan["frame_codes"][::5], codes.double()[plan["stops"][:-1]])
