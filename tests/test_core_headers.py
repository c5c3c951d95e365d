"""The arithmetic headers the HIP kernels share with the twin (csrc/*_core.h, core_fn.h) are plain C++: each compiles on its own with
g++, without a HIP header in reach, in a translation unit that includes it twice."""
import glob
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "shapegan_amd", "csrc")


def test_core_headers_are_plain_cpp_with_include_guards(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    headers = sorted(glob.glob(os.path.join(CSRC, "*_core.h"))) + [os.path.join(CSRC, "core_fn.h")]
    assert {os.path.basename(h) for h in headers} >= {"mesh_core.h", "raymarch_core.h", "pointcloud_core.h", "raster_core.h", "core_fn.h"}
    for h in headers:
        tu = tmp_path / (os.path.basename(h) + ".cpp")
        tu.write_text('#include "%s"\n#include "%s"\n' % (h, h))
        r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(tu)], capture_output=True, text=True)
        assert r.returncode == 0, "%s does not stand alone as plain C++:\n%s" % (os.path.basename(h), r.stderr)
