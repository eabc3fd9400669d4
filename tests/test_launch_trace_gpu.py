"""The launches of the token step and of the prefill, pinned: which ops go out, in which order, on which weights and which
buffers (tests/launch_trace.py says what a record holds).  tests/golden/decode_launch_trace.json was recorded on the commit
before LMEngine's decode step was split into one method per block kind; a pull request that changes the step on purpose
regenerates it (``python tests/launch_trace.py > tests/golden/decode_launch_trace.json`` on a GPU) and the diff of that file is
the statement of what changed.  Parity tests cannot see a swapped scratch buffer that happens to hold the same values, or a block
that quietly took the generic path; this one can."""
import json
import os

import pytest

import launch_trace as LT

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_launch_trace.json")) as f:
    GOLDEN = json.load(f)


def test_golden_covers_the_cases():
    assert set(GOLDEN) == set(LT.CASES)
    for name, case in LT.CASES.items():
        assert set(GOLDEN[name]) == set(case[4]), name


@pytest.mark.parametrize("name", list(LT.CASES))
def test_launches_match_golden(dev, name):
    out, res = LT.run_case(dev, LT.CASES[name])
    assert not isinstance(res, Exception), res
    got = json.loads(json.dumps(out))
    for phase, want in GOLDEN[name].items():
        for i, (g, w) in enumerate(zip(got[phase], want)):
            assert g == w, f"{name} / {phase}: record {i} differs"
        assert len(got[phase]) == len(want), f"{name} / {phase}: {len(got[phase])} launches, golden has {len(want)}"


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selection_launch_trace.json")) as f:
    SELECT_GOLDEN = json.load(f)


def test_selection_golden_covers_the_cases():
    assert set(SELECT_GOLDEN) == set(LT.SELECT_CASES)
    for name in LT.SELECT_CASES:
        assert set(SELECT_GOLDEN[name]) == {"first", "step"} and all(SELECT_GOLDEN[name].values()), name


@pytest.mark.parametrize("name", list(LT.SELECT_CASES))
def test_selection_launches_match_golden(dev, name):
    """The selection ops of the first token and of one cached step under every selection mode and the combinations that take
    another path (tests/golden/selection_launch_trace.json: recorded on the commit before the modes became one SelectionPlan)."""
    got = json.loads(json.dumps(LT.run_select_case(dev, LT.SELECT_CASES[name])))
    for phase, want in SELECT_GOLDEN[name].items():
        for i, (g, w) in enumerate(zip(got[phase], want)):
            assert g == w, f"{name} / {phase}: record {i} differs"
        assert len(got[phase]) == len(want), f"{name} / {phase}: {len(got[phase])} launches, golden has {len(want)}"


def test_w8_refusal_comes_before_the_first_launch(dev):
    """W8A16 on a grouped block whose adapter has no e4m3 operand (r = 256 at d = 1024): decode() refuses while it plans the
    step, with nothing of that step enqueued.  (Planning packs the e4m3 weights first: those quantize_rows_fp8 launches read
    fresh weight tensors, never a buffer of the step, and no op of the step is a quantisation.)"""
    out, res = LT.run_case(dev, LT.REFUSAL)
    assert isinstance(res, NotImplementedError), res
    assert "W8A16 decode needs adapter projections with K % 1024 == 0" in str(res)
    packing = [r for r in out["decode"] if r["op"] == "quantize_rows_fp8" and r["x"].startswith("?")]
    assert packing and [r for r in out["decode"] if r not in packing] == []
