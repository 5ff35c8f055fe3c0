"""The graph walker and the fake tensors of tools/layer_calls.py against the real autograd engine: the training cases of the layers,
``forward_pooled``, ``MyLinear`` and ``UpConv`` whose route depends on no size threshold, run on REAL CUDA tensors through
``loss.backward()`` against the same recording stand-in for the library (nothing is launched, no stream is created), print what the
fake-tensor run of the same shapes prints -- and that is what the CPU fixture holds for those cases (tests/golden/layer_calls,
tests/test_layer_calls_cpu.py)."""
import lzma
import os
import subprocess
import sys

import pytest

from test_layer_calls_cpu import GOLDEN, ROOT
from test_op_calls_cpu import blocks


@pytest.mark.gpu
def test_real_engine_prints_what_the_walker_prints():
    got = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "layer_calls.py"), ROOT, "--real"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, universal_newlines=True)
    assert got.returncode == 0, got.stderr[-4000:]
    fake, _, real = got.stdout.partition("#### fake\n")[2].partition("#### real\n")
    strip = lambda text: [(h, b.split("\n# ")[0]) for h, b in blocks(text)]
    fake, real = strip(fake), strip(real)
    assert len(real) == len(fake) > 60, (len(real), len(fake))
    bad = [(r, f) for r, f in zip(real, fake) if r != f]
    assert not bad, "%d of %d cases differ between the real engine and the walker, e.g.\n%s\nwalked:\n%s" % (len(bad), len(real), bad[0][0][1], bad[0][1][1])
    with lzma.open(os.path.join(GOLDEN, "calls.txt.xz"), "rt") as f:
        want = dict(strip(f.read()))
    bad = [(h, b) for h, b in fake if want.get(h) != b]
    assert not bad, "%d of %d cases differ from the fixture, e.g.\n%s\nrecorded:\n%s" % (len(bad), len(fake), bad[0][1], want.get(bad[0][0]))
