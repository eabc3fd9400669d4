"""transformers' sampler, host side (DESIGN.md "transformers' sampler"): the host statements ``top_k_filter_ties``,
``nucleus_filter`` and ``min_p_filter`` (magma_amd/sampling.py) -- the sort-free fixed-point rule the device kernel shares --
against transformers' own chained warpers, the argument checks of generate(), and the pins the GPU tests read."""
import os

import pytest
import torch

import warper_cases as W
from magma_amd import sampling as S

PINS_PATH = os.path.join(os.path.dirname(__file__), "golden", "warper_pins.pt")


@pytest.mark.parametrize("V", [1000, 50258])
@pytest.mark.parametrize("kind", W.TIE_FREE)
def test_host_chain_equals_transformers_on_tie_free_rows(kind, V):
    pytest.importorskip("transformers")
    x = W.make_rows(kind, 6, V)
    assert all(x[r].unique().numel() == V for r in range(6))
    fired = 0
    for prm in W.GRID:
        want, got = W.transformers_kept(x, *prm), W.host_kept(x, *prm)
        assert torch.equal(got, want), (kind, V, prm, int((got != want).sum()))
        fired += int((~got).any())
    assert fired >= len(W.GRID) // 2              # the rules really dropped something


@pytest.mark.parametrize("V", [1000, 50258])
def test_host_chain_equals_transformers_per_value_on_tied_rows(V):
    """torch.sort / torch.topk order equal values arbitrarily: per distinct value the NUMBER of survivors is what is defined."""
    pytest.importorskip("transformers")
    x = W.make_rows("bf16", 6, V)
    assert x[0].unique().numel() < V - V // 8              # there are ties
    for prm in W.GRID:
        want, got = W.transformers_kept(x, *prm), W.host_kept(x, *prm)
        for r in range(6):
            assert W.count_diff(x[r], got[r], want[r]) == 0, (V, prm, r)


def test_edge_rows():
    pytest.importorskip("transformers")
    x = W.make_rows("randn", 4, 1000)
    top = x.argmax(1)
    only_max = torch.zeros_like(x, dtype=torch.bool).scatter_(1, top[:, None], True)
    # top_p so small that only the maximum stays
    assert torch.equal(W.host_kept(x, 1.0, 0, 1e-6, 0.0), only_max)
    assert torch.equal(W.transformers_kept(x, 1.0, 0, 1e-6, 0.0), only_max)
    # top_p = 1.0 and top_p = 0 are both off
    assert bool(W.host_kept(x, 0.7, 0, 1.0, 0.0).all()) and bool(W.host_kept(x, 0.7, 0, 0.0, 0.0).all())
    # min_p = 1.0 keeps only the maxima -- all of them
    y = x.clone()
    y[:, 5] = y.max(1).values
    maxima = y == y.max(1, keepdim=True).values
    assert int(maxima.sum()) == 8
    assert torch.equal(W.host_kept(y, 1.3, 0, 0.0, 1.0), maxima)
    assert torch.equal(W.transformers_kept(y, 1.3, 0, 1.0, 1.0), maxima)
    # k = 1
    assert torch.equal(W.host_kept(x, 0.7, 1, 0.9, 0.05), only_max)
    assert torch.equal(W.transformers_kept(x, 0.7, 1, 0.9, 0.05), only_max)
    # a row with V - 1 entries at -inf
    z = torch.full((2, 1000), float("-inf"))
    z[0, 333], z[1, 0] = 1.5, -2.0
    for prm in ((0.7, 0, 0.9, 0.0), (1.0, 40, 0.3, 0.05), (1.3, 0, 1.0, 1.0)):
        assert torch.equal(W.host_kept(z, *prm), ~torch.isneginf(z)), prm
        assert torch.equal(W.transformers_kept(z, *prm), ~torch.isneginf(z)), prm
    # top-k ties at the k-th value all stay (the reference's filter keeps exactly k)
    t = torch.arange(20.0)[None, :].clone()
    t[0, 3:8] = 15.0                                   # values 19 18 17 16 | 15 15 15 15 15 15 | ...: k = 6 straddles the ties
    kept = W.host_kept(t, 1.0, 6, 0.0, 0.0)
    assert int(kept.sum()) == 10 and bool(kept[0, 3:8].all()) and bool(kept[0, 15])
    assert torch.equal(kept, W.transformers_kept(t, 1.0, 6, 1.0, 0.0))
    assert int((~torch.isneginf(S.top_k_filter(t, 6))).sum()) == 6


def test_nucleus_differs_from_the_reference_rule():
    """The case the opt-in exists for: on a peaked row the reference's "top-p" drops nothing (a no-op whenever the
    top-1 probability is at least 1 - top_p), nucleus 0.9 keeps fewer than 10 tokens."""
    x = W.make_rows("peaked", 6, 50258)
    ref = S.top_p_filter(x, 0.9)
    assert int(torch.isneginf(ref).sum()) == 0
    new = S.nucleus_filter(x, 0.9, 1.0)
    kept = (~torch.isneginf(new)).sum(1)
    assert int(kept.max()) < 10 and int(kept.min()) >= 1
    assert bool(new.gather(1, x.argmax(1, keepdim=True)).isfinite().all())
    # and at the default call's values on an ordinary row: thousands of tokens go
    y = W.make_rows("randn3", 2, 50258)
    assert int(torch.isneginf(S.top_p_filter(y / 0.7, 0.9)).sum()) == 0
    assert int(torch.isneginf(S.nucleus_filter(y, 0.9, 0.7)).sum(1).min()) > 40000


def test_check_sampler_args():
    assert S.check_sampler_args() is None
    assert S.check_sampler_args("reference", 0.0, 0.9) is None
    assert S.check_sampler_args("reference", 0, 7.0) is None              # the reference's sampler keeps its own top_p handling
    assert S.check_sampler_args("transformers", 0.0, 0.9) == {"min_p": 0.0}
    assert S.check_sampler_args("transformers", 0.05, 0.0) == {"min_p": 0.05}
    assert S.check_sampler_args("transformers", 1, 1.0) == {"min_p": 1.0}
    for bad in ("nucleus", None, "", 1):
        with pytest.raises(ValueError, match="sampler"):
            S.check_sampler_args(bad)
    for bad in (-0.1, 1.5, float("nan"), "0.1", True, None):
        with pytest.raises(ValueError, match="min_p"):
            S.check_sampler_args("transformers", bad)
    with pytest.raises(ValueError, match="min_p"):
        S.check_sampler_args("reference", 0.05)
    for bad in (-0.1, 1.5, float("nan"), None):
        with pytest.raises(ValueError, match="top_p"):
            S.check_sampler_args("transformers", 0.0, bad)


class _HostLM(torch.nn.Module):
    """An LM object without device token selection: fixed logits per step."""

    def __init__(self, logits):
        super().__init__()
        self.table = logits

    def forward(self, input_ids=None, inputs_embeds=None, use_cache=True, past_key_values=None, **kw):
        from types import SimpleNamespace
        step = 0 if past_key_values is None else past_key_values + 1
        B = (inputs_embeds if inputs_embeds is not None else input_ids).shape[0]
        out = {"logits": self.table[step][None, None, :].repeat(B, 1, 1), "past_key_values": step}
        ns = SimpleNamespace(**out)
        ns.get = out.get
        return ns


class _HostModel(torch.nn.Module):
    eos_token, image_token = 0, 1

    def __init__(self, logits):
        super().__init__()
        self.lm = _HostLM(logits)


def test_generate_host_chain_and_argument_errors():
    """An LM object without device token selection gets the chain on the host: only kept tokens are ever drawn."""
    V, steps = 64, 5
    table = W.make_rows("randn3", steps, V)
    model = _HostModel(table)
    emb = torch.zeros(16, 2, 8)
    torch.manual_seed(0)
    out = S.generate(model, emb, max_steps=steps, temperature=0.7, top_k=0, top_p=0.5, decode=False, stop_on_eos=False,
                     sampler="transformers", min_p=0.1)
    assert out.shape == (16, 2 + steps)
    for t in range(steps):
        kept = W.host_kept(table[t:t + 1], 0.7, 0, 0.5, 0.1)[0]
        assert 1 <= int(kept.sum()) < V // 2
        assert bool(kept[out[:, 2 + t]].all()), t
    # top_p = 1e-6: greedy
    out = S.generate(model, emb, max_steps=steps, temperature=0.7, top_p=1e-6, decode=False, stop_on_eos=False,
                     sampler="transformers")
    assert torch.equal(out[:, 2:], table.argmax(1)[None, :].repeat(16, 1))
    with pytest.raises(ValueError, match="sampler"):
        S.generate(model, emb, max_steps=2, sampler="hf")
    with pytest.raises(ValueError, match="min_p"):
        S.generate(model, emb, max_steps=2, min_p=0.1)
    with pytest.raises(ValueError, match="min_p"):
        S.generate(model, emb, max_steps=2, temperature=0.0, sampler="transformers", min_p=0.1)
    with pytest.raises(ValueError, match="min_p"):
        S.generate(model, emb, max_steps=2, num_beams=2, sampler="transformers", min_p=0.1)
    with pytest.raises(ValueError, match="top_p"):
        S.generate(model, emb, max_steps=2, sampler="transformers", top_p=1.5)
    with pytest.raises(TypeError):
        S.generate(model, emb, 2, 0.7, 0, 0.9, None, False, True, None, None, None, 1, 1.0, False, 1, False, None, False,
                   "transformers")                                          # keyword-only


def test_pins_match_their_generator_and_transformers():
    pins = torch.load(PINS_PATH, weights_only=False)
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_warper_golden",
                                                  os.path.join(os.path.dirname(PINS_PATH), "make_warper_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    x = pins["logits"]
    assert torch.equal(x, gen.pin_rows()) and x.shape == (8, 1000)
    assert [tuple(p) for p in pins["params"]] == [tuple(p) for p in W.GRID]
    assert os.path.getsize(PINS_PATH) < 128 * 1024
    nt = pins["tie_free_rows"]
    kept = W.unpack(pins["kept"], x.shape[1])
    for i, prm in enumerate(W.GRID):                          # the host statement against the pins: needs no transformers
        got = W.host_kept(x, *prm)
        assert torch.equal(got[:nt], kept[i, :nt]), prm
        for r in range(nt, x.shape[0]):
            assert W.count_diff(x[r], got[r], kept[i, r]) == 0, (prm, r)
    pytest.importorskip("transformers")
    for i, prm in enumerate(W.GRID):
        assert torch.equal(W.transformers_kept(x, *prm), kept[i]), prm
