"""Every C-ABI call the Python op wrappers make -- entry point, arguments in order, workspace and output shapes -- and every refusal with
its text, against tests/golden/ops/, without a GPU (tools/op_calls.py: the wrappers of sonet_hip/ops.py on fake CUDA tensors against a
recording stand-in for the library).  calls.txt.xz is the output of the tool on a checkout of the commit BEFORE the wrappers' building
blocks were merged, calls.summary.txt its outline per wrapper: they are that commit's behaviour and are never regenerated from the tree
under test.  tightened.txt holds the cases this tree refuses although that commit launched them (scale / shift / bias of the wrong length
or dtype, a pos / weight / x of the pooled-layer backward of the wrong shape, which the kernels would have read past or misread): each replaces the recorded case of the same call and must be a refusal."""
import difflib
import lzma
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ops")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def blocks(text):
    """-> [(header line, whole block)] of the ``== call`` cases; the ``# section`` lines stay with the block they follow."""
    out = []
    for line in text.splitlines():
        if line.startswith("== "):
            out.append([line, line])
        elif out:
            out[-1][1] += "\n" + line
    return out


def expected():
    """The recorded text with the tightened cases in place of the recorded ones -> (text, number of cases replaced)."""
    with lzma.open(os.path.join(GOLDEN, "calls.txt.xz"), "rt") as f:
        want = f.read()
    tight = dict(blocks(open(os.path.join(GOLDEN, "tightened.txt")).read()))
    recorded = dict(blocks(want))
    for head, block in tight.items():
        assert head in recorded, "tightened.txt names a case the recording does not hold: " + head
        assert "\n  !! " not in recorded[head], "a tightened case was a refusal already: " + head
        lines = block.split("\n")
        assert len(lines) == 2 and lines[1].startswith("  !! SonetHipError: "), block
    first = want.split("== ", 1)[0]
    # (a ``# section`` line that follows a replaced case stays)
    return first + "\n".join(tight[h] + b[len(b.split("\n# ")[0]):] if h in tight else b for h, b in blocks(want)) + "\n", want, len(tight)


def test_wrappers_call_as_recorded():
    import op_calls
    got = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "op_calls.py"), ROOT], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True)
    assert got.returncode == 0, got.stderr[-4000:]
    want, recorded, _ = expected()
    # the committed outline is the outline of the committed text: neither fixture moved without the other
    assert op_calls.summarise(recorded) == open(os.path.join(GOLDEN, "calls.summary.txt")).read()
    if got.stdout != want:
        diff = list(difflib.unified_diff(want.splitlines(), got.stdout.splitlines(), "recorded", "this tree", n=1, lineterm=""))
        outline = list(difflib.unified_diff(op_calls.summarise(want).splitlines(), op_calls.summarise(got.stdout).splitlines(),
                                            "recorded outline", "this tree", n=0, lineterm=""))
        pytest.fail("%d differing lines against tests/golden/ops/calls.txt.xz\n%s\n%s" % (len(diff), "\n".join(outline[:60]), "\n".join(diff[:80])))
