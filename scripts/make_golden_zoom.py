"""Records tests/golden/zoom_scipy.npz: small inputs and what scipy.ndimage makes of them in float64, so that the definition of K20
(tests/zoom_reference.py) stays tied to scipy.ndimage.zoom / map_coordinates on machines without scipy.

    python scripts/make_golden_zoom.py

Inputs are noise clamped to [-1, 1].  zoom at (5,7,4) x 3, 8^3 x 2, (2,3,4) x 4 and 9^3 x 2.5; order 1 at (5,7,4) x 3; map_coordinates at
200 in-domain points of a (6,5,7) grid."""
import os

import numpy as np
from scipy import ndimage

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "zoom_scipy.npz")
ZOOMS = (("a", (5, 7, 4), 3, 3), ("b", (8, 8, 8), 2, 3), ("c", (2, 3, 4), 4, 3), ("d", (9, 9, 9), 2.5, 3), ("e", (5, 7, 4), 3, 1))


def noise(rng, shape):
    return np.clip(rng.normal(0, 0.7, size=shape), -1, 1)


def main():
    rng = np.random.default_rng(20)
    data = {}
    for name, shape, factor, order in ZOOMS:
        grid = noise(rng, shape)
        data["zoom_%s_in" % name] = grid
        data["zoom_%s_factor" % name] = np.float64(factor)
        data["zoom_%s_order" % name] = np.int64(order)
        data["zoom_%s_out" % name] = ndimage.zoom(grid, factor, order=order)
    grid = noise(rng, (6, 5, 7))
    points = rng.uniform(0, 1, size=(200, 3)) * (np.array(grid.shape) - 1)
    points[:8] = np.array([[0, 0, 0], [5, 4, 6], [5, 0, 3.25], [2, 4, 6], [0.5, 2, 6], [5, 4, 0], [3, 3, 3], [4.75, 3.5, 5.5]])
    data["sample_in"] = grid
    data["sample_points"] = points
    data["sample_out"] = ndimage.map_coordinates(grid, points.T, order=3, mode="constant", cval=1.0)
    np.savez_compressed(OUT, **data)
    print("wrote %s: %d bytes" % (os.path.normpath(OUT), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
