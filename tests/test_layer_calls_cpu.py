"""What the model layers call -- every C-ABI call in order with its arguments, the side stream's enter / keep / reads / join(defer=...),
the aten operators that move data between the launches, what comes back and every refusal with its text -- against tests/golden/layer_calls/,
without a GPU (tools/layer_calls.py: the modules and autograd nodes of models/layers.py on fake CUDA tensors against the recording stand-in
for the library, the backward pass walked node by node).  calls.txt.xz is the output of the tool on a checkout of the commit BEFORE the
layers' building blocks were merged, calls.summary.txt its outline per case family: they are that commit's behaviour and are never
regenerated from the tree under test.  There is no exceptions file: this tree prints that text."""
import difflib
import lzma
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "layer_calls")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_layers_call_as_recorded():
    import op_calls
    got = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "layer_calls.py"), ROOT], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True)
    assert got.returncode == 0, got.stderr[-4000:]
    with lzma.open(os.path.join(GOLDEN, "calls.txt.xz"), "rt") as f:
        want = f.read()
    # the committed outline is the outline of the committed text: neither fixture moved without the other
    assert op_calls.summarise(want) == open(os.path.join(GOLDEN, "calls.summary.txt")).read()
    if got.stdout != want:
        diff = list(difflib.unified_diff(want.splitlines(), got.stdout.splitlines(), "recorded", "this tree", n=1, lineterm=""))
        outline = list(difflib.unified_diff(op_calls.summarise(want).splitlines(), op_calls.summarise(got.stdout).splitlines(),
                                            "recorded outline", "this tree", n=0, lineterm=""))
        pytest.fail("%d differing lines against tests/golden/layer_calls/calls.txt.xz\n%s\n%s" % (len(diff), "\n".join(outline[:60]), "\n".join(diff[:80])))
