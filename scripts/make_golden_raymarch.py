"""Writes tests/golden/raymarch_chairs.npz: images of the reference's own rendering/raymarching.py:render_image, run on CPU with
the chairs SDFNet weights (tests/golden/sdfnet_chairs_weights.npz) and two seeded latent codes.

    python scripts/make_golden_raymarch.py [--reference DIR]

Needs the reference source tree; imports it unchanged, with three import-time shims:
  * a stub `rendering` package whose __path__ is the reference's rendering/ directory (its __init__ imports pygame / OpenGL);
  * rendering.math.get_rotation_matrix rebuilt on Rotation.as_matrix (SciPy >= 1.6 has no as_dcm), before raymarching imports it;
  * PIL.Image.ANTIALIAS = Image.LANCZOS (removed in Pillow 10).
The hit points and shadow values come from wrapping the reference's get_shadows (its first call in a render gets the hit points,
the second the ground points).
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SETTINGS = dict(radius=1.6, sdf_offset=-0.045, vertical_cutoff=1)   # create_plot.py:778,793,809,834
RESOLUTION = 32


def latents():
    return (torch.randn(2, 128, generator=torch.Generator().manual_seed(31)) * 0.5).float()


def load_reference(ref):
    for m in ("trimesh", "skimage", "skimage.measure"):
        sys.modules.setdefault(m, types.ModuleType(m))
    os.chdir(tempfile.mkdtemp(prefix="shapegan_ref_"))   # the reference's util creates directories in the CWD
    sys.path.insert(0, ref)
    from PIL import Image
    Image.ANTIALIAS = Image.LANCZOS
    pkg = types.ModuleType("rendering")
    pkg.__path__ = [os.path.join(ref, "rendering")]
    sys.modules["rendering"] = pkg
    import rendering.math as rmath
    from scipy.spatial.transform import Rotation

    def get_rotation_matrix(angle, axis='y'):
        matrix = np.identity(4)
        matrix[:3, :3] = Rotation.from_euler(axis, angle, degrees=True).as_matrix()
        return matrix
    rmath.get_rotation_matrix = get_rotation_matrix
    import rendering.raymarching as rm
    from model.sdf_net import SDFNet
    return rm, SDFNet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SHAPEGAN_REFERENCE", "reference"))
    args = ap.parse_args()
    rm, SDFNet = load_reference(os.path.abspath(args.reference))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    w = np.load(os.path.join(GOLDEN, "sdfnet_chairs_weights.npz"))
    net = SDFNet(device="cpu")
    net.load_state_dict({k: torch.from_numpy(w[k]) for k in w.files})
    net.eval()
    z = latents()
    calls = []
    inner = rm.get_shadows

    def get_shadows(sdf_net, points, *a, **k):
        out = inner(sdf_net, points, *a, **k)
        calls.append((np.array(points, dtype=np.float32), np.array(out, dtype=np.float32)))
        return out
    rm.get_shadows = get_shadows
    out = {"camera_position": rm.camera_position, "light_position": rm.light_position, "latents": z.numpy(),
           "resolution": np.array(RESOLUTION)}
    for ssaa in (1, 2):
        for i in range(z.shape[0]):
            calls.clear()
            img = rm.render_image(net, z[i], resolution=RESOLUTION, ssaa=ssaa, **SETTINGS)
            out["image_ssaa%d_%d" % (ssaa, i)] = np.asarray(img)
            (hp, hs), (gp, gs) = calls
            out["hits_ssaa%d_%d" % (ssaa, i)] = hp
            out["hit_shadows_ssaa%d_%d" % (ssaa, i)] = hs
            out["ground_points_ssaa%d_%d" % (ssaa, i)] = gp
            out["ground_shadows_ssaa%d_%d" % (ssaa, i)] = gs
            print("ssaa", ssaa, "latent", i, "hits", hp.shape[0], "ground", gp.shape[0], flush=True)
    calls.clear()
    out["image_default_0"] = np.asarray(rm.render_image(net, z[0], resolution=RESOLUTION))
    out["hits_default_0"] = calls[0][0]
    path = os.path.join(GOLDEN, "raymarch_chairs.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
