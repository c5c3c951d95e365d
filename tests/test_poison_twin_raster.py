"""The rasteriser's twin under poison (tests/raster_poison_bodies.py): every output written in full, no stale scratch read."""
import pytest

import raster_poison_bodies as B


def test_stage_bodies_under_poison():
    B.check_bodies("cpu")


@pytest.mark.parametrize("name,width", B.FORMS)
def test_outputs_written_and_repeatable(name, width):
    B.check_outputs_and_repeat("cpu", name, width)


def test_renderer_under_poison():
    B.check_renderer("cpu")
