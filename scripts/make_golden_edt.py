"""Records tests/golden/edt_scipy.npz: small masks and what scipy.ndimage.distance_transform_edt makes of them in float64, so that the
definition of K21 (tests/edt_reference.py) stays tied to scipy on machines without it.

    python scripts/make_golden_edt.py

Masks (packed as bits) of (5,7,4), 8^3, (1,9,3), (16,16,16) random at several densities, a ball in 12^3 and a single zero in a corner of
(6,5,9); each with unit sampling and with sampling (1, 2, 0.5)."""
import os

import numpy as np
from scipy import ndimage

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "edt_scipy.npz")
SAMPLING = (1.0, 2.0, 0.5)


def masks():
    rng = np.random.default_rng(21)
    out = {"a": rng.random((5, 7, 4)) < 0.7, "b": rng.random((8, 8, 8)) < 0.9, "c": rng.random((1, 9, 3)) < 0.6,
           "d": rng.random((16, 16, 16)) < 0.97}
    ax = np.arange(12) - 5.5
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    out["e"] = x * x + y * y + z * z < 20.0
    corner = np.ones((6, 5, 9), dtype=bool)
    corner[5, 0, 8] = False
    out["f"] = corner
    return out


def main():
    data = {}
    for name, mask in masks().items():
        data["%s_shape" % name] = np.array(mask.shape, dtype=np.int64)
        data["%s_bits" % name] = np.packbits(mask.reshape(-1))
        data["%s_unit" % name] = ndimage.distance_transform_edt(mask)
        data["%s_sampled" % name] = ndimage.distance_transform_edt(mask, sampling=SAMPLING)
    data["sampling"] = np.array(SAMPLING)
    np.savez_compressed(OUT, **data)
    print("wrote %s: %d bytes" % (os.path.normpath(OUT), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
