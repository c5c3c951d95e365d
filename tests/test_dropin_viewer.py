"""The reference's train_wgan.py WITHOUT `nogui`: it imports `rendering.MeshRenderer`, creates one and shows it the current sample
(train_wgan.py:22-24, :79-80).  Through shapegan_amd.dropin that is the headless renderer; with --viewer-dir it leaves PNGs behind.
Skipped where the reference checkout is absent, as tests/test_dropin.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dropin_cases as cases

REF = os.environ.get("SHAPEGAN_REFERENCE_DIR", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "train_wgan.py")),
                                     reason="reference scripts not present (set SHAPEGAN_REFERENCE_DIR)")


@needs_reference
def test_train_wgan_with_its_viewer(tmp_path, monkeypatch):
    from PIL import Image
    from shapegan_amd import dropin
    from shapegan_amd.rendering import MeshRenderer
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    case = cases.BY_NAME["wgan_b4"]
    cases.prepare(case)
    shots = tmp_path / "shots"
    # the command line of the issue, in a process of its own: the class-level default must not leak into this one
    script = ("import sys, torch\n"
              "torch.manual_seed(1)\n"
              "from shapegan_amd import dropin\n"
              "src = open(sys.argv[1]).read().replace('BATCH_SIZE = 64', 'BATCH_SIZE = 4')\n"
              "open('train_wgan.py', 'w').write(src)\n"
              "sys.argv = ['dropin', '--epochs', '1', '--viewer-dir', sys.argv[2], 'train_wgan.py']\n"
              "sys.exit(dropin.main())\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    done = subprocess.run([sys.executable, "-c", script, os.path.join(REF, "train_wgan.py"), str(shots)], env=env, capture_output=True,
                          text=True, timeout=600)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    pngs = sorted(os.listdir(shots))
    assert pngs and pngs[0] == "000000.png"
    image = np.asarray(Image.open(shots / pngs[0]))
    assert image.shape == (800, 800, 3) and (image != 255).any(), "the snapshot is uniformly white"
    assert MeshRenderer.snapshot_directory is None and "rendering" in dropin.ALIASES
