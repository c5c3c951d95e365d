"""The rasteriser's HIP kernels under poison (tests/raster_poison_bodies.py, the pattern of tests/test_gpu_unwritten.py): every output
written in full, integer scratch that starts as zeros never leaves its buffer, nothing stale read, two runs bit-identical."""
import pytest

import raster_poison_bodies as B

pytestmark = pytest.mark.gpu


def test_stage_bodies_under_poison():
    B.check_bodies("cuda")


@pytest.mark.parametrize("name,width", B.FORMS)
def test_outputs_written_and_repeatable(name, width):
    B.check_outputs_and_repeat("cuda", name, width)


def test_renderer_under_poison():
    B.check_renderer("cuda")
