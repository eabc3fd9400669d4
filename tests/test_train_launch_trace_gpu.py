"""The launches of the LM half of the training step, pinned: which ops _lm_forward and _lm_backward send out, in which order, on
which weights and buffers (tests/launch_trace.py says what a record holds and how a tensor is named).
tests/golden/train_launch_trace.json was recorded on the commit before MagmaEngine's block forward / backward were split into one
helper per block kind; a pull request that changes the step on purpose regenerates it (``python tests/launch_trace.py train >
tests/golden/train_launch_trace.json`` on a GPU) and the diff of that file is the statement of what changed.  The recorder does not
see torch-side work (index_select, index_copy_, copy_, add_), so the golden also holds the bits of the loss and a SHA-256 of every
gradient that reproduced in every recording run (its header lists the others: sums formed with fp32 atomics in the trunk)."""
import functools
import json
import os

import pytest

import launch_trace as LT

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_launch_trace.json")) as f:
    GOLDEN = json.load(f)

# (mlp, attn, attention) of blocks 0 and 1: DESIGN.md, "The training block kinds"
KINDS = {
    "v1": ("cat", "none", "rows"), "v1_nocat": ("serial", "none", "rows"), "v1_allrows": ("cat", "none", "rows"),
    "v1_recompute": ("cat", "none", "rows"), "v2": ("serial", "serial", "rows"), "attn_only": ("none", "serial", "rows"),
    "no_adapters": ("none", "none", "rows"), "parallel": ("parallel", "parallel", "rows"), "ln_gelu_erf": ("serial", "none", "rows"),
    "lm_trainable": ("serial", "none", "rows"), "fp8_row": ("serial", "none", "rows"), "fp8_mx": ("serial", "none", "fp8"),
    "fp8_all": ("fp8", "none", "fp8"),
}


@functools.lru_cache(maxsize=None)
def run(dev, name):
    """One forward and backward of the case, shared by the two tests."""
    out, eng = LT.run_train_case(dev, LT.TRAIN_CASES[name])
    return out, bool(eng._ad8_cache)


def test_golden_covers_the_cases():
    assert set(GOLDEN["cases"]) == set(LT.TRAIN_CASES) == set(KINDS)


@pytest.mark.parametrize("name", list(LT.TRAIN_CASES))
def test_launches_loss_and_gradients_match_golden(dev, name):
    got, want = run(dev, name)[0], GOLDEN["cases"][name]
    for i, (g, w) in enumerate(zip(got["records"], want["records"])):
        assert g == w, f"{name}: record {i} differs"
    assert len(got["records"]) == len(want["records"]), f"{name}: {len(got['records'])} launches, golden has {len(want['records'])}"
    assert got["loss"] == want["loss"], f"{name}: loss bits {got['loss']}, golden {want['loss']}"
    assert set(want["grads"]) | set(GOLDEN["header"]["unstable"]) >= set(got["grads"]) >= set(want["grads"])
    assert any(".adapter." in n for n in want["grads"]) == (name != "no_adapters") and "image_prefix.proj.weight" in want["grads"]
    for n, digest in want["grads"].items():
        assert got["grads"][n] == digest, f"{name}: gradient of {n} differs"


@pytest.mark.parametrize("name", list(LT.TRAIN_CASES))
def test_block_kinds(dev, name):
    """sv["kind"] as the backward read it from the tape (under recompute: from the rebuilt entry) is the DESIGN table's."""
    out, ad8 = run(dev, name)
    assert out["kinds"] == [list(KINDS[name])] * 2
    assert ad8 == (name == "fp8_all")
    if name == "fp8_all":
        # the MX adapter chain's backward: block 1 runs it, the bottom block (prefix rows only) takes the serial adapter's
        used = {r["w"]["w"] for r in out["records"] if isinstance(r.get("w"), dict) and str(r["w"]["w"]).startswith("_ad8_cache")}
        assert {"_ad8_cache[1][1]['up_t']", "_ad8_cache[1][1]['dn_t']", "_ad8_cache[0][1]['up']"} <= used
        assert not {"_ad8_cache[0][1]['up_t']", "_ad8_cache[0][1]['dn_t']"} & used
