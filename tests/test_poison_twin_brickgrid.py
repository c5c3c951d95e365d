"""The narrow-band entry points of the twin under poison (tests/brickgrid_forms.py): the grid written in full, lists up to their
counts, nothing stale read, a small call after a large one."""
import brickgrid_forms as F


def test_brickgrid_writes_everything():
    F.check_poison("cpu")
