"""The decoder's up-convolution kernels (so-net_amd/csrc/upconv.hip, upconv_bwd.hip, upconv_wgrad.hip) bit for bit: every output of every
case of tools/upconv_bits.py -- the forward with its pack and trailer, ReLU on and off; the input gradient with its pack; the weight
gradient -- has the sha256 recorded in tests/golden/upconv_bits.json, twice in a row.  The case table, what each case reaches and the
inputs (continuous values from integer arithmetic, no library's random stream) are in tools/upconv_bits.py; the fixture was recorded on an
MI355X from the tree before the family's building blocks were shared, so a helper that reorders a product chain or a flush fails here.
The float64 comparisons of tests/test_gpu_upconv*.py stay the tests of what the kernels compute; this one holds their bits."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "so-net_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import upconv_bits as U  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(U.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_case_table(recorded):
    assert sorted(recorded) == sorted(U.NAMES)


@pytest.mark.parametrize("name", U.NAMES)
def test_upconv_bits(name, recorded):
    first, second = U.run_case(name), U.run_case(name)
    assert first == recorded[name], "%s: outputs %s differ from the recording" % (
        name, [i for i, (a, b) in enumerate(zip(first, recorded[name])) if a != b] or "(count)")
    assert second == first, "%s: not the same bits run to run" % name


@pytest.mark.parametrize("a, b", U.SAME_BITS)
def test_the_load_path_does_not_change_the_bits(a, b, recorded):
    """the weight gradient's 16-byte loads and its element-wise loads: the same values in the same order"""
    assert recorded[a] == recorded[b]
    assert U.run_case(a) == U.run_case(b)
