"""shapegan_amd/traversal.py on the device: the frame identity and the command line (bodies: tests/test_traversal.py)."""
import pytest

import test_traversal as B

pytestmark = pytest.mark.gpu


def test_traversal_frames_equal_the_viewer_loop():
    B.frames_body("cuda")


def test_command_line(tmp_path, capsys):
    B.cli_body("cuda", tmp_path, capsys)
