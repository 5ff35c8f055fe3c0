"""The dispatch of the layer launchers -- which kernel instantiation, grid, block and LDS size every entry point, shape, CU count and
SONET_* knob gets, and what is refused with which message -- against tests/golden/launch/, without a GPU (tools/launch_log.py: the host
halves of so-net_amd/csrc compiled host-only against a recording stand-in for the runtime).  The fixtures are the output of the tool on a
checkout of the commit BEFORE the host-side refactor of the launchers: NAME.txt.xz the whole text (lzma, 27,000 lines), NAME.summary.txt its
outline per section and entry point.  They are that commit's behaviour, and a change of dispatch is a reviewed diff of the outline (with
the cases this test prints), never a regeneration from the tree under test."""
import difflib
import lzma
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch")
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.parametrize("name, flags", [("product", []), ("variants", ["--variants"])])
def test_launchers_dispatch_as_recorded(name, flags):
    import launch_log
    got = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "launch_log.py"), ROOT] + flags, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, universal_newlines=True)
    assert got.returncode == 0, got.stderr[-4000:]
    with lzma.open(os.path.join(GOLDEN, name + ".txt.xz"), "rt") as f:
        want = f.read()
    # the committed outline is the outline of the committed text: neither fixture moved without the other
    assert launch_log.summarise(want) == open(os.path.join(GOLDEN, name + ".summary.txt")).read()
    if got.stdout != want:
        diff = list(difflib.unified_diff(want.splitlines(), got.stdout.splitlines(), "recorded", "this tree", n=1, lineterm=""))
        outline = list(difflib.unified_diff(launch_log.summarise(want).splitlines(), launch_log.summarise(got.stdout).splitlines(),
                                            "recorded outline", "this tree", n=0, lineterm=""))
        pytest.fail("%d differing lines against tests/golden/launch/%s.txt.xz\n%s\n%s" % (len(diff), name, "\n".join(outline[:60]), "\n".join(diff[:80])))
