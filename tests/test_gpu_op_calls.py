"""A fake CUDA tensor answers the op wrappers' questions as a real one does: the layer family of tools/op_calls.py at B = 2, 32 -> 64 and
48 + 16 -> 64, L in {8, 33}, run on REAL CUDA tensors against the same recording stand-in for the library (nothing is launched), prints
the very cases the CPU fixture holds (tests/golden/ops, tests/test_op_calls_cpu.py).  Only the second device is left out."""
import os
import subprocess
import sys

import pytest

from test_op_calls_cpu import ROOT, blocks, expected


@pytest.mark.gpu
def test_real_tensors_print_the_recorded_cases():
    got = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "op_calls.py"), ROOT, "--real"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, universal_newlines=True)
    assert got.returncode == 0, got.stderr[-4000:]
    want = dict((h, b.split("\n# ")[0]) for h, b in blocks(expected()[0]))
    cases = blocks(got.stdout)
    assert len(cases) > 800, len(cases)
    bad = [(h, b) for h, b in cases if want.get(h) != b]
    assert not bad, "%d of %d cases differ from the fixture, e.g.\n%s\nrecorded:\n%s" % (len(bad), len(cases), bad[0][1], want.get(bad[0][0]))
