"""GPU (-m gpu): the host forward makes the launches tests/golden/forward_trace.json lists -- the same entry points with the same integer
and float arguments and the same null pattern, in the same order -- and computes the same bytes (tests/forward_trace.py).  The golden
file was written before the host code was restructured; a change that needs it regenerated has changed behaviour."""
import pytest

import forward_trace as FT

pytestmark = pytest.mark.gpu


def test_the_golden_file_lists_exactly_the_scenarios():
    assert sorted(FT.load_golden()) == sorted(FT.SCENARIOS)


@pytest.mark.parametrize("name", list(FT.SCENARIOS))
def test_forward_trace(name):
    want = FT.load_golden()[name]
    trace, dig = FT.run_scenario(name)
    for n, (got, exp) in enumerate(zip(trace, want["trace"])):
        assert got == exp, f"call {n} of {len(want['trace'])}: {got!r}, golden {exp!r}"
    assert len(trace) == len(want["trace"])
    if want["digest"] is not None:                        # (null: the scenario is not bit-reproducible on the device; its trace is pinned)
        assert dig == want["digest"]
