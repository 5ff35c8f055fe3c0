"""The inputs of tools/pooled_bits.py (tests/test_gpu_pooled_bits.py, tests/golden/pooled_bits.json) make the fmas round: the check the
tool documents, run without a GPU, so that a changed hash or case table cannot quietly turn the recording into one of exact sums."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pooled_bits as P  # noqa: E402


def test_the_inputs_of_the_bits_fixture_make_the_fmas_round():
    worst = P.check()
    assert set(worst) == set(P.CHECK_FLOORS)
    for kind, floor in P.CHECK_FLOORS.items():
        assert worst[kind] >= floor, (kind, worst[kind], floor)
