"""The library's translation units (vanrijn_amd/build.py): the list the build compiles is the directory's, the
render units are the ones that include the render kernel, and each of them instantiates one camera mode.
Compiles nothing."""
import os
import re
import subprocess
import sys

from vanrijn_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit_text(name):
    with open(os.path.join(build.CSRC, name)) as f:
        return f.read()


def test_sources_are_the_directory():
    on_disk = [f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp"))]
    assert len(build.SOURCES) == len(set(build.SOURCES))
    assert set(build.SOURCES) == set(on_disk)


def test_render_sources_include_the_kernel():
    printed = subprocess.check_output([sys.executable, os.path.join(ROOT, "vanrijn_amd", "build.py"),
                                       "--print-render-sources"], text=True).split()
    including = [s for s in build.SOURCES if '#include "vr_render_kernel.h"' in unit_text(s)]
    assert printed == build.RENDER_SOURCES
    assert sorted(printed) == sorted(including) and len(printed) == 3
    assert build.SOURCES[:3] == printed  # the long compiles start first


def test_each_camera_unit_instantiates_its_mode():
    for name in build.RENDER_SOURCES:
        found = re.findall(r"^template\s+\w+\s+(\w+)<(\d+)>\(", unit_text(name), re.M)
        assert found == [("launch_render_class", re.fullmatch(r"vr_render_cam(\d)\.hip", name).group(1))], name
