"""The rasteriser stage by stage on the C++ twin against tests/raster_reference.py (float64 / exact integers).

Every stage's reference starts from the PREVIOUS stage's kernel output, so an ulp upstream cannot pass for an error downstream:
  setup       clip coordinates within 8 u sum|M v| of float64, snapped coordinates within one unit of the float64 rounding, flags and
              dropped counts exact on a hand mesh with one triangle of each kind, ground level exact (-1 for an empty shape);
  bins        counts, offsets, the list of non-empty tiles and every tile's list AS A SET equal the reference's;
  visibility  sample by sample: something is drawn exactly where the brute-force covering set is non-empty, and for the hand meshes and
              the sphere the covering set itself is checked triangle by triangle (each triangle drawn as a shape of its own: its
              coverage mask must equal the integer reference's).  The winner equals the reference's wherever the two nearest
              float64 depths differ by more than tau = 26 u (Z_a + Z_b) (raster_reference.depth_tau derives it); samples inside
              tau are left out and may be at most 2 % of the covered ones;
  shade       every byte within 1 of the float64 colour, floor and background included, except samples where one of the reference's
              36 shadow comparisons is within raster_reference.shadow_tau of flipping (at most 2 %).
The same bodies run on the GPU (tests/test_gpu_raster.py) and under poison.

Shares left out, measured with the float64 reference alone on these inputs (records of the twin; samples 48 / 40 wide, shadow map 64):
  visibility  0 % in every case, camera and light pass (covered samples: quad 576 / 400, offscreen 594 / 413, sliver 12 / 7,
              sphere16 213 / 150, torus16 191 / 133, two_spheres16 174 / 125, noise16 1303 / 907; light pass 0 .. 475)
  shade       quad 0 / 0 %, offscreen 0.13 / 0.06 %, sliver 0 / 0 %, sphere16 0.39 / 0.44 %, torus16 0.13 / 0.13 %,
              two_spheres16 0.39 / 0.25 %, noise16 1.30 / 0.94 % (the light's depth range over the model is 0.006, so 36 comparisons
              per sample against a bound of a few 1e-7 leave about a percent on a surface as rough as the noise grid)
(printed by every run: `pytest -s`).
"""
import functools

import numpy as np
import pytest
import torch

import raster_reference as RR
from shapegan_amd import mesh as M
from shapegan_amd.rendering import raster
from shapegan_amd.rendering.math import get_camera_transform

CAMERA_VP = get_camera_transform(1.4 * 2, 147, 20, project=True)
LIGHT_VP = get_camera_transform(6, 147, 50, project=True)
SHADOW = 64
VIEWS = [(48, 1), (40, 1), (24, 2)]          # (size, ssaa): the sample grid is size * ssaa wide
CASES = ["quad", "offscreen", "sliver", "sphere16", "torus16", "two_spheres16", "noise16"]
SINGLE_TRIANGLE_CASES = ["quad", "offscreen", "sliver", "sphere16"]
CAP = 0.02


def unproject(ndc, vp=CAMERA_VP):
    """World points whose NDC under vp are `ndc` [n,3]."""
    h = np.concatenate([np.asarray(ndc, dtype=np.float64), np.ones((len(ndc), 1))], axis=1) @ np.linalg.inv(vp).T
    return (h[:, :3] / h[:, 3:4]).astype(np.float32)


def _grid(R):
    ax = torch.linspace(-1, 1, R)
    return torch.meshgrid(ax, ax, ax, indexing="ij")


def sdf_grid(name, R=16):
    x, y, z = _grid(R)
    if name == "sphere":
        return (x * x + y * y + z * z).sqrt() - 0.6
    if name == "torus":
        return (((x * x + z * z).sqrt() - 0.55) ** 2 + y * y).sqrt() - 0.22
    if name == "two_spheres":
        a = ((x + 0.25) ** 2 + y * y + z * z).sqrt() - 0.45
        b = ((x - 0.3) ** 2 + (y - 0.1) ** 2 + (z - 0.1) ** 2).sqrt() - 0.4
        return torch.minimum(a, b)
    if name == "noise":
        return torch.rand((R, R, R), generator=torch.Generator().manual_seed(5)) * 2 - 1
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_soup(name):
    """(positions [T,3,3], normals or None, tri_offsets) as CPU tensors."""
    if name == "quad":          # two front-facing triangles sharing the edge (-0.5, -0.5) -- (0.5, 0.5)
        p = unproject([(-0.5, -0.5, 0.6), (0.5, -0.5, 0.6), (0.5, 0.5, 0.6), (-0.5, -0.5, 0.6), (0.5, 0.5, 0.6), (-0.5, 0.5, 0.6)])
    elif name == "offscreen":
        p = unproject([(-1.5, -0.2, 0.5), (0.3, -0.6, 0.7), (0.1, 0.7, 0.6)])
    elif name == "sliver":      # thinner than a sample everywhere
        p = unproject([(-0.9, -0.5, 0.6), (0.9, 0.52, 0.6), (-0.9, -0.48, 0.6)])
    else:
        grid = sdf_grid(name[:-2])
        if name == "two_spheres16":
            # two separate meshes in one soup, so that the surfaces really pass through each other
            x, y, z = _grid(16)
            a = ((x + 0.25) ** 2 + y * y + z * z).sqrt() - 0.45
            b = ((x - 0.3) ** 2 + (y - 0.1) ** 2 + (z - 0.1) ** 2).sqrt() - 0.4
            soups = [raster.pack(M.marching_cubes(g, spacing=2.0 / 16, origin=-1.0), smooth=True) for g in (a, b)]
            pos, nrm = torch.cat([s.positions for s in soups]), torch.cat([s.normals for s in soups])
            return pos, nrm, torch.tensor([0, pos.shape[0]], dtype=torch.int64)
        soup = raster.pack(M.marching_cubes(grid, spacing=2.0 / 16, origin=-1.0), smooth=name != "noise16")
        return soup.positions, soup.normals, soup.tri_offsets
    pos = torch.from_numpy(p.reshape(-1, 3, 3))
    return pos, None, torch.tensor([0, pos.shape[0]], dtype=torch.int64)


def soup_on(name, device):
    pos, nrm, off = case_soup(name)
    return raster.Soup(pos.to(device), None if nrm is None else nrm.to(device), off.to(device))


def view_arrays(v):
    """A View's tensors as numpy copies (None stays None)."""
    out = {}
    for k in ("recs", "flags", "clip", "dropped", "ground", "tile_counts", "tile_offsets", "active", "lists", "id", "depth"):
        t = getattr(v, k, None)
        out[k] = None if t is None else t.cpu().numpy().copy()
    out["nactive"], out["ntx"], out["nty"] = getattr(v, "nactive", None), v.ntx, v.nty
    return out


def bins_as_sets(a):
    n = a["tile_counts"].size
    return {g: frozenset(a["lists"][a["tile_offsets"][g]:a["tile_offsets"][g + 1]].tolist()) for g in range(n)
            if a["tile_offsets"][g + 1] > a["tile_offsets"][g]}


PARAMS = raster.shading_params(CAMERA_VP, LIGHT_VP, (0.8, 0.1, 0.1), (1, 1, 1, 1))


def draw(name, width, device):
    """All stages of one case: the light pass at SHADOW, the camera pass at width, the shaded samples."""
    soup = soup_on(name, device)
    light = raster.draw_view(soup, LIGHT_VP, SHADOW, SHADOW, cull_back=False, shadow=True, clip=True)
    cam = raster.draw_view(soup, CAMERA_VP, width, width, cull_back=True, ground=True, clip=True)
    image = raster.shade(soup, cam, light.depth, cam.ground, PARAMS)
    return soup, view_arrays(light), view_arrays(cam), image.cpu().numpy().copy()


# ---- setup ------------------------------------------------------------------------------------------------------------------------
def hand_mesh():
    """One triangle of each kind under CAMERA_VP at 48 x 48, then an empty shape, then a second shape of two kept triangles."""
    eye = np.linalg.inv(get_camera_transform(1.4 * 2, 147, 20))[:3, 3].astype(np.float32)
    front = unproject([(-0.4, -0.4, 0.5), (0.4, -0.4, 0.5), (0.0, 0.5, 0.5)])
    back = front[[0, 2, 1]]
    zero = unproject([(-0.2, 0.1, 0.5), (0.3, 0.2, 0.5), (0.3, 0.2, 0.5)])
    near = np.stack([front[0], front[1], eye])
    guard = unproject([(900.0, 0.0, -0.9), (0.4, -0.4, 0.5), (0.0, 0.5, 0.5)])      # ~55 units to the side, just behind the near distance
    far_off = unproject([(3.0, 3.0, 0.5), (3.5, 3.0, 0.5), (3.2, 3.6, 0.5)])
    tris = np.stack([front, back, zero, near, guard, far_off, front + np.float32(0.01), front - np.float32(0.02)])
    expected = [0, RR.BACK, RR.ZERO_AREA, RR.NEAR, RR.GUARDED, RR.OFFSCREEN, 0, 0]
    return torch.from_numpy(tris), torch.tensor([0, 6, 6, 8], dtype=torch.int64), expected


def body_setup(device):
    pos, off, expected = hand_mesh()
    soup = raster.Soup(pos.to(device), None, off.to(device))
    out = {}
    for cull, vp, W in ((True, CAMERA_VP, 48), (False, LIGHT_VP, SHADOW), (True, CAMERA_VP, 40)):
        a = view_arrays(raster.setup(soup, vp, W, W, cull_back=cull, ground=True, clip=True))
        out[cull, W] = a
        clip, bound, X, Y, near_flag, guard_flag = RR.setup(pos.numpy(), vp, W, W, cull, raster.NEAR)
        assert np.all(np.abs(a["clip"].astype(np.float64) - clip) <= bound), "clip coordinates beyond 8 u sum|M v|"
        x, y, z, iw, box = RR.unpack_records(a["recs"])
        # the reference's own decisions, from ITS rounding of the float64 window coordinates: this mesh keeps every decision far from
        # its threshold (the zero-area triangle repeats a corner), so they are exact
        xr, yr = (np.nan_to_num(np.rint(c), nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64) for c in (X, Y))
        flags, _ = RR.flags_from_snapped(xr, yr, near_flag, guard_flag, cull, W, W)
        assert np.array_equal(a["flags"], flags)
        kept = (a["flags"] & raster.DROPPED) == 0
        assert np.all(np.abs(x[kept] - np.rint(X[kept])) <= 1) and np.all(np.abs(y[kept] - np.rint(Y[kept])) <= 1)
        # the sample box is an integer function of the kernel's own snapped coordinates (dropped: zeros and the empty box)
        _, ref_box = RR.flags_from_snapped(x, y, near_flag, guard_flag, cull, W, W)
        assert np.array_equal(box, ref_box)
        if cull:
            assert a["flags"].tolist() == expected
            assert a["dropped"].tolist() == [4, 0, 0]
        else:
            assert a["flags"][1] == 0 and a["dropped"].tolist()[1:] == [0, 0]          # the shadow pass culls nothing
        assert np.all(a["recs"][~kept][:, :12] == 0) and np.all(a["recs"][~kept][:, 12:] == (1, 1, 0, 0))
        w = clip[:, :, 3]
        assert np.allclose(z[kept], (clip[:, :, 2] / w)[kept], atol=1e-5) and np.allclose(iw[kept], 1 / w[kept], rtol=1e-5)
        g = a["ground"]
        assert g[0] == pos[:6, :, 1].min().item() and g[1] == -1.0 and g[2] == pos[6:, :, 1].min().item()
    return out


def test_setup_twin():
    body_setup("cpu")


def test_near_distance_comes_from_the_projection_matrix():
    assert abs(raster.NEAR - 0.1) < 1e-6


# ---- bins ---------------------------------------------------------------------------------------------------------------------------
def check_bins(a, tri_offsets):
    x, y, _, _, box = RR.unpack_records(a["recs"])
    ref = RR.tile_sets(a["flags"], box, tri_offsets, a["ntx"], a["nty"])
    ntiles = a["ntx"] * a["nty"]
    ref = {(s * a["nty"] + ty) * a["ntx"] + tx: frozenset(v) for (s, ty, tx), v in ref.items()}
    counts = a["tile_counts"].reshape(-1)
    assert counts.size == ntiles * (len(tri_offsets) - 1)
    assert {g: int(c) for g, c in enumerate(counts) if c} == {g: len(v) for g, v in ref.items()}
    assert np.array_equal(a["tile_offsets"], np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]))
    assert a["nactive"] == len(ref) and a["active"][:a["nactive"]].tolist() == sorted(ref)
    assert a["lists"].shape[0] == int(counts.sum())
    assert bins_as_sets(a) == ref
    return counts


# ---- visibility ---------------------------------------------------------------------------------------------------------------------
def check_visibility(a, tri_offsets, width, shadow, what):
    """a: one view's arrays.  Returns the share of covered samples left out."""
    left_out = covered = 0
    for s in range(len(tri_offsets) - 1):
        count, id1, z1, z2, tau = RR.visibility(a["recs"], a["flags"], int(tri_offsets[s]), int(tri_offsets[s + 1]), width, width)
        depth = a["depth"][s]
        drawn = depth != 1.0 if shadow else a["id"][s] >= 0
        assert np.array_equal(drawn, count > 0), what + ": drawn samples differ from the non-empty covering sets"
        assert np.all(depth[count == 0] == 1.0)
        with np.errstate(invalid="ignore"):          # inf - inf where nothing is drawn
            sure = (count > 0) & (z2 - z1 > tau)
        left_out += int(((count > 0) & ~sure).sum())
        covered += int((count > 0).sum())
        if shadow:
            assert np.all(np.abs(depth[sure] - (0.5 * z1[sure] + 0.5)) <= 0.5 * tau[sure] + RR.U), what
        else:
            assert np.array_equal(a["id"][s][sure], id1[sure]), what + ": winner differs outside tau"
            assert np.all(np.abs(depth[sure] - z1[sure]) <= tau[sure]), what
            # inside tau the winner is still one of the near-ties: the gap (<= tau) plus its own rounding (<= tau)
            unsure = (count > 0) & ~sure
            assert np.all(np.abs(depth[unsure] - z1[unsure]) <= 2 * tau[unsure])
    share = left_out / max(covered, 1)
    print("%s: %d covered samples, %.3f %% inside tau" % (what, covered, 100 * share))
    assert share <= CAP, what
    return share


def check_single_triangles(name, width, device, cull_back, vp):
    """Every triangle as a shape of its own: its drawn samples are its covering set, exactly."""
    pos, _, _ = case_soup(name)
    T = pos.shape[0]
    soup = raster.Soup(pos.to(device), None, torch.arange(T + 1, dtype=torch.int64, device=device))
    a = view_arrays(raster.draw_view(soup, vp, width, width, cull_back=cull_back, shadow=not cull_back))
    total = np.zeros((width, width), dtype=np.int64)
    for t in range(T):
        ref = RR.coverage_single(a["recs"], a["flags"], t, width, width)
        got = a["id"][t] == t if cull_back else a["depth"][t] != 1.0
        assert np.array_equal(got, ref), "%s: coverage of triangle %d" % (name, t)
        if cull_back:
            assert np.all(a["id"][t][~ref] == -1)
        total += ref
    return total


def body_case(name, width, device):
    soup, light, cam, image = draw(name, width, device)
    off = soup.tri_offsets.cpu().numpy()
    counts = check_bins(cam, off)
    check_bins(light, off)
    if name == "noise16":
        assert counts.max() > raster.CHUNK, "the noise case must spill an LDS chunk"
    check_visibility(cam, off, width, False, "%s/%d camera" % (name, width))
    check_visibility(light, off, SHADOW, True, "%s/%d light" % (name, width))
    check_shade(soup, cam, light, image, width, "%s/%d" % (name, width))
    return light, cam, image


def check_shade(soup, cam, light, image, width, what):
    pos = soup.positions.cpu().numpy()
    nrm = None if soup.normals is None else soup.normals.cpu().numpy()
    colour, fragile = RR.shade(pos, nrm, cam["recs"], cam["id"][0], cam["depth"][0], light["depth"][0], float(cam["ground"][0]), PARAMS,
                               width, width)
    diff = np.abs(image[0].astype(np.float64) - colour * 255.0)
    bad = (diff > 1.0 + 1e-9).any(axis=2) & ~fragile
    share = fragile.mean()
    print("%s shade: %.3f %% fragile, largest difference elsewhere %.3f" % (what, 100 * share, diff[~fragile].max()))
    assert not bad.any(), "%s: %d samples differ by more than one level, first at %s" % (what, bad.sum(), np.argwhere(bad)[0])
    assert share <= CAP, what
    assert (image[0] != 255).any() and (image[0] == 255).all(axis=2).any()


@pytest.mark.parametrize("size,ssaa", VIEWS)
@pytest.mark.parametrize("name", CASES)
def test_stages_twin(name, size, ssaa):
    body_case(name, size * ssaa, "cpu")


@pytest.mark.parametrize("name", SINGLE_TRIANGLE_CASES)
def test_covering_sets_twin(name):
    for width in (48, 40):
        total = check_single_triangles(name, width, "cpu", True, CAMERA_VP)
        if name == "quad":
            # the quad's interior, the shared diagonal included, is owned exactly once
            assert total.max() == 1 and total.sum() > 0.2 * width * width
            d = np.arange(width)
            on_diagonal = total[width - 1 - d, d]
            assert on_diagonal[width // 4 + 1:3 * width // 4 - 1].tolist() == [1] * (3 * width // 4 - 1 - width // 4 - 1)
        if name == "sliver":
            assert 0 < total.sum() < width
    check_single_triangles(name, SHADOW, "cpu", False, LIGHT_VP)
