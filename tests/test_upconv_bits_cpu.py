"""The case table of tools/upconv_bits.py (tests/test_gpu_upconv_bits.py, tests/golden/upconv_bits.json) is what it says, without a
GPU: unique names, every case reaches what its row claims (tile, chunk, flush, slice and live-pair counts from the extents ops.py exports
and upconv_wgrad_ref.plan), and the inputs are order-sensitive -- the f32 sum of a case's partial products differs run backwards -- so
that a changed hash or shape cannot quietly turn the recording into one of exact sums."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import upconv_bits as U  # noqa: E402


def test_the_case_table_of_the_bits_fixture_is_what_it_says():
    assert U.check() == []
