"""The dispatch of the layer launchers -- which kernel instantiation, grid, block and LDS size every entry point, shape, CU count and
SONET_* knob gets, and what is refused with which message -- against tests/golden/launch/, without a GPU (tools/launch_log.py: the host
halves of so-net_amd/csrc compiled host-only against a recording stand-in for the runtime).  The fixtures are the output of the tool on a
checkout of the commit BEFORE the host-side refactor of the launchers: NAME.txt.xz the whole text (lzma, 27,000 lines), NAME.summary.txt its
outline per section and entry point.  They are that commit's behaviour, and a change of dispatch is a reviewed diff of the outline (with
the cases this test prints), never a regeneration from the tree under test.

The sections "bn passes: ..." at the end of either fixture (the BatchNorm / ReLU passes, the coefficient kernels, the eval-mode head kernels
and the pooled sparse gradient) were appended later, recorded from the parent of the refactor of those passes; the sections in front of
them are byte for byte what they were.  That refactor merged kernels: tests/golden/launch/renamed.txt lists old name -> new name (names
only), the tool prints a kernel under the first old name listed for it, and where the recording tells two merged kernels apart the texts
are compared case by case with the names resolved (launch_log.expand) -- every case, return code, message, kernel, grid, block and LDS
size still has to agree.

The sections "upconv: ..." behind them (the decoder's up-convolutions: pack sizes, pack kernels, forward, input gradient, weight gradient
and its workspace size) were appended the same way, recorded from the parent of that family's refactor.  The family reads no knob, so the
variants fixture holds the half only where the variants build differs from the product build: nowhere."""
import difflib
import lzma
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_renamed_holds_names_only():
    """tests/golden/launch/renamed.txt: two mangled kernel names per line, nothing else; every old name is one the recordings hold."""
    import re
    recorded = set()
    for name in ("product", "variants"):
        with lzma.open(os.path.join(GOLDEN, name + ".txt.xz"), "rt") as f:
            recorded |= {l.split(" ", 1)[1] for l in f.read().split("\n") if re.match(r"K\d+ ", l)}
    lines = [l for l in open(os.path.join(GOLDEN, "renamed.txt")).read().split("\n") if l]
    assert lines
    for l in lines:
        old, new = l.split(" ")
        assert re.fullmatch(r"_Z\w+", old) and re.fullmatch(r"_Z\w+", new) and old in recorded, l


@pytest.mark.parametrize("name, flags", [("product", []), ("variants", ["--variants"])])
def test_launchers_dispatch_as_recorded(name, flags):
    import launch_log
    got = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "launch_log.py"), ROOT, "--bn", "--upconv"] + flags, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, universal_newlines=True)
    assert got.returncode == 0, got.stderr[-4000:]
    with lzma.open(os.path.join(GOLDEN, name + ".txt.xz"), "rt") as f:
        want = f.read()
    # the committed outline is the outline of the committed text: neither fixture moved without the other
    assert launch_log.summarise(want) == open(os.path.join(GOLDEN, name + ".summary.txt")).read()
    # case by case with the kernel names resolved (through renamed.txt): every case, return code, message, kernel, grid, block, LDS size
    want_cases, got_cases = launch_log.expand(want), launch_log.expand(got.stdout)
    if got_cases != want_cases:
        diff = list(difflib.unified_diff(want_cases, got_cases, "recorded", "this tree", n=1, lineterm=""))
        outline = list(difflib.unified_diff(launch_log.summarise(want).splitlines(), launch_log.summarise(got.stdout).splitlines(),
                                            "recorded outline", "this tree", n=0, lineterm=""))
        pytest.fail("%d differing lines against tests/golden/launch/%s.txt.xz\n%s\n%s" % (len(diff), name, "\n".join(outline[:60]), "\n".join(diff[:80])))
    # ... and the sections recorded before the bn passes were appended are the recording byte for byte, tables and digests included
    cut = want.index("== bn passes: kernels and refusal texts\n")
    assert got.stdout[:cut] == want[:cut]
