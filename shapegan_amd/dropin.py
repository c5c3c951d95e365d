"""Runs the reference's own training scripts on the native modules, unmodified.

    python -m shapegan_amd.dropin /path/to/shapegan/train_wgan.py nogui
    python -m shapegan_amd.dropin --epochs 1 /path/to/shapegan/train_autoencoder.py classic nogui
    python -m shapegan_amd.dropin --epochs 1 --viewer-dir shots /path/to/shapegan/train_wgan.py

Without `nogui` the scripts create a `rendering.MeshRenderer` and show it the current sample (train_wgan.py:22-24,79-80).  The
native one (shapegan_amd.rendering) is headless; `--viewer-dir DIR` makes it leave a PNG in DIR for every shape it is shown, by
setting the class-level default `MeshRenderer.snapshot_directory` before the script runs.

The reference has no plugin interface: its scripts import `model.*`, `util` and `datasets` by name (train_wgan.py:13-17,
train_autoencoder.py:6,18-20, train_sdf_autodecoder.py:13-14, train_hybrid_progressive_gan.py:15-19,
train_hybrid_wgan.py:14-19).  `install_aliases()` registers the shapegan_amd mirrors under exactly those names, so
`from model.gan import Generator, Discriminator` resolves to the HIP-backed classes while everything else in the script —
the loop, stock `torch.optim` optimizers, `zero_grad()`, `clip_weights()`, `generate()`, `save()`/`load()`, the
`DataLoader` over `VoxelDataset` — stays the reference's own code.

`run_script` executes a script file in a fresh `__main__` namespace.  The scripts loop `for epoch in count():` forever
and run `train()` at import time; `epochs=N` bounds that by substituting `itertools.count` for the duration of the run
(nothing in the script text is edited for it).  `replace` applies literal text substitutions to the source before it is
compiled — used for the one line of train_sdf_autodecoder.py that no longer runs on torch >= 1.5
(`indices / POINTCLOUD_SIZE` yields floats; the intended floor division is `//`) and by tests that
shrink module-level constants such as BATCH_SIZE.
"""
import itertools
import os
import sys

ALIASES = {
    "model": "shapegan_amd.model",
    "model.gan": "shapegan_amd.model.gan",
    "model.autoencoder": "shapegan_amd.model.autoencoder",
    "model.progressive_gan": "shapegan_amd.model.progressive_gan",
    "model.sdf_net": "shapegan_amd.model.sdf_net",
    "model.point_sdf_net": "shapegan_amd.model.point_sdf_net",
    "util": "shapegan_amd.util",
    "datasets": "shapegan_amd.datasets",
    "rendering": "shapegan_amd.rendering",
    "rendering.math": "shapegan_amd.rendering.math",
    "rendering.raymarching": "shapegan_amd.rendering.raymarching",
}

# train_sdf_autodecoder.py:78 — true division of an int64 index tensor; torch >= 1.5 returns floats, which cannot index
SDF_AUTODECODER_FIX = {"model_indices = indices / POINTCLOUD_SIZE": "model_indices = indices // POINTCLOUD_SIZE"}


def install_aliases(make_dirs=True):
    """Registers the native mirrors under the reference's module names.  Returns the dict of displaced sys.modules
    entries so that `remove_aliases` can restore them.  The reference's `util` creates plots/ models/ data/ in the CWD
    when imported (util.py:11-13) and the scripts rely on it (`open("plots/...")`); make_dirs reproduces that here."""
    import importlib
    displaced = {}
    for name, target in ALIASES.items():
        module = importlib.import_module(target)
        if name in sys.modules and sys.modules[name] is not module:
            displaced[name] = sys.modules[name]
        sys.modules[name] = module
    if make_dirs:
        for d in ("plots", "models", "data"):
            os.makedirs(d, exist_ok=True)
    return displaced


def remove_aliases(displaced=None):
    for name in ALIASES:
        sys.modules.pop(name, None)
    if displaced:
        sys.modules.update(displaced)


class _BoundedCount(object):
    """itertools.count stand-in: `count(start)` yields `epochs` values and stops."""

    def __init__(self, epochs):
        self.epochs = epochs

    def __call__(self, start=0, step=1):
        return iter(range(start, start + self.epochs * step, step))


def run_script(path, argv=(), epochs=None, replace=None, aliases=True):
    """Executes the script at `path` as __main__ with sys.argv = [path, *argv] in the current working directory.
    Returns the script's global namespace (its modules, optimizers, histories).  With aliases=False the imports are
    left alone (used to run the same script on the reference's own modules when they are importable)."""
    with open(path, "r") as fh:
        source = fh.read()
    for old, new in (replace or {}).items():
        if old not in source:
            raise ValueError("run_script: %r does not occur in %s" % (old, path))
        source = source.replace(old, new)
    code = compile(source, path, "exec")
    namespace = {"__name__": "__main__", "__file__": path, "__builtins__": __builtins__}
    displaced = install_aliases() if aliases else None
    saved_argv, saved_count = sys.argv, itertools.count
    sys.argv = [path] + list(argv)
    if epochs is not None:
        itertools.count = _BoundedCount(epochs)
    try:
        exec(code, namespace)
    finally:
        itertools.count = saved_count
        sys.argv = saved_argv
        if aliases:
            remove_aliases(displaced)
    return namespace


def main():
    args = sys.argv[1:]
    epochs = None
    while args and args[0] in ("--epochs", "--viewer-dir"):
        if args[0] == "--epochs":
            epochs = int(args[1])
        else:
            from shapegan_amd.rendering import MeshRenderer
            MeshRenderer.snapshot_directory = os.path.abspath(args[1])
        args = args[2:]
    if not args:
        print(__doc__)
        return 2
    script = args[0]
    replace = SDF_AUTODECODER_FIX if os.path.basename(script) == "train_sdf_autodecoder.py" else None
    run_script(script, args[1:], epochs=epochs, replace=replace)
    return 0


if __name__ == "__main__":
    sys.exit(main())
