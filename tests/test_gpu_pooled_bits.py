"""The pooled-layer backward (so-net_amd/csrc/pooled_bwd.hip) bit for bit: every output of every case of tools/pooled_bits.py -- the
sparse input gradient with f32 output, bf16 output and on the matrix cores, the weight gradient through its four entry points -- has the
sha256 recorded in tests/golden/pooled_bits.json, twice in a row.  The case table, what each case reaches and the inputs (integer
arithmetic, no library's random stream) are in tools/pooled_bits.py; the fixture was recorded on an MI355X from the tree before the
family's building blocks were shared, so a helper that reorders an fma chain or a store fails here.  The float64 comparisons of
tests/test_gpu_parity.py stay the tests of what the kernels compute; this one holds their bits."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "so-net_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pooled_bits as P  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(P.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_case_table(recorded):
    assert sorted(recorded) == sorted(P.NAMES)


@pytest.mark.parametrize("name", P.NAMES)
def test_pooled_backward_bits(name, recorded):
    first, second = P.run_case(name), P.run_case(name)
    assert first == recorded[name], "%s: outputs %s differ from the recording" % (
        name, [i for i, (a, b) in enumerate(zip(first, recorded[name])) if a != b] or "(count)")
    assert second == first, "%s: not the same bits run to run" % name
