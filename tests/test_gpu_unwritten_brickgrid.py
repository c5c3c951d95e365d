"""The narrow-band kernels under poison (tests/brickgrid_forms.py, the pattern of tests/test_gpu_unwritten.py): the grid written in
full, lists up to their counts, nothing stale read, two runs bit-identical, a small call after a large one."""
import pytest

import brickgrid_forms as F

pytestmark = pytest.mark.gpu


def test_brickgrid_writes_everything():
    F.check_poison("cuda")
