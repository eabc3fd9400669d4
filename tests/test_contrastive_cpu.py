"""Contrastive search on the host (DESIGN.md "Contrastive search"): contrastive_rank against a literal restatement, every shared
kernel case decided under the derived bound, contrastive_search on a toy LM with a real (cache-less) forward, the argument
checks, and the defaults' plan keys.  No GPU."""
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import contrastive_cases as CC
from magma_amd.sampling import (check_contrastive_args, contrastive_margin, contrastive_rank, contrastive_search, generate)


# ------------------------------------------------------------------------------------------------------- contrastive_rank
def _restated(ctx, ctx_len, hidden, p, alpha):
    """The rule, literally: normalise, matmul, mask, max, (1 - a) p - a pen, argmax."""
    c = F.normalize(ctx.double(), dim=-1, eps=0.0).nan_to_num(0.0)
    h = F.normalize(hidden.double(), dim=-1, eps=0.0).nan_to_num(0.0)
    cos = h @ c.transpose(1, 2)
    mask = torch.arange(ctx.shape[1])[None, None, :] >= ctx_len.long()[:, None, None]
    pen = cos.masked_fill(mask, -math.inf).max(-1).values
    score = (1 - alpha) * p.double() - alpha * pen
    return score.argmax(-1), score, pen


@pytest.mark.parametrize("d,k,T,adv", CC.kernel_cases())
def test_rank_equals_restatement_and_case_is_decided(d, k, T, adv):
    case = CC.sim_case(d, k, T, CC.case_seed(d, k, T, adv), adversarial=adv)
    sel, score, pen, gap = CC.reference(case)
    r_sel, r_score, r_pen = _restated(case["ctx"], case["ctx_len"], case["hidden"], case["p"], case["alpha"])
    assert torch.equal(sel, r_sel)
    assert torch.allclose(score, r_score, rtol=0, atol=1e-12) and torch.allclose(pen, r_pen, rtol=0, atol=1e-12)
    # the check, done here, that the GPU tests' inputs keep the reference inside the condition
    assert float(gap.min()) > CC.gap_bound(case["alpha"], d), (float(gap.min()), CC.gap_bound(case["alpha"], d))
    n0 = int(case["ctx_len"][0])
    if adv in ("equal", "last_valid"):
        assert abs(float(pen[0, 0]) - 1.0) < 1e-9
    if adv == "scaled":                   # 3 x is rounded to bf16 element by element: 1 up to that rounding
        assert abs(float(pen[0, 0]) - 1.0) < 2.0 ** -16
    if adv == "zero_row":
        assert float(pen[0, k - 1]) == 0.0 and bool(torch.isfinite(pen).all())
    if adv == "past_len":                 # the row one past the length equals the candidate: seen, it would give cosine 1
        assert float(pen[0, 0]) < 0.99
        full = case["ctx_len"].clone()
        full[0] = n0 + 1
        assert abs(float(contrastive_rank(case["ctx"], full, case["hidden"], case["p"], case["alpha"])[2][0, 0]) - 1.0) < 1e-9


def test_rank_first_of_equal_scores_and_empty_context():
    ctx = torch.randn(1, 4, 8)
    hidden = torch.randn(1, 1, 8).repeat(1, 3, 1)
    p = torch.tensor([[0.2, 0.2, 0.2]])
    sel, score, pen = contrastive_rank(ctx, [4], hidden, p, 0.5)
    assert int(sel) == 0 and float(score[0, 0]) == float(score[0, 2])
    sel, score, pen = contrastive_rank(ctx, [0], hidden, torch.tensor([[0.1, 0.3, 0.2]]), 0.5)
    assert int(sel) == 1 and bool((pen == 0).all())


# ----------------------------------------------------------------------------------------------------------------- the toy LM
class ToyLM:
    """A deterministic causal LM without a cache: h_t = tanh(A mean(e_<=t) + M e_t), logits_t = h_t U + copy * <e_t, E_v> / d.  With
    ``copy`` large the most probable next token is the last one again: greedy decoding loops."""

    def __init__(self, V=40, d=24, seed=0, copy=0.0):
        g = torch.Generator().manual_seed(seed)
        self.E = torch.randn(V, d, generator=g)
        self.A, self.M = torch.randn(d, d, generator=g) / d ** 0.5, torch.randn(d, d, generator=g) / d ** 0.5
        self.U = torch.randn(d, V, generator=g) / d ** 0.5
        self.copy, self.V, self.d = copy, V, d

    def forward(self, e):                                   # (R, T, d) -> hidden (R, T, d), logits (R, T, V)
        mean = e.cumsum(1) / torch.arange(1, e.shape[1] + 1)[None, :, None]
        h = torch.tanh(mean @ self.A + e @ self.M)
        return h, h @ self.U + self.copy * (e @ self.E.T) / self.d

    def driver(self, prompts, lengths, k):
        """(step callback, prompt hidden (B, S, d), first logits (B, V)) for contrastive_search: the callback keeps every row's
        embedded prefix (its 'cache'), re-gathered by ``parents``."""
        B, S, _ = prompts.shape
        lens = [S] * B if lengths is None else list(lengths)
        rows = [prompts[b, : lens[b]] for b in range(B) for _ in range(k)]
        h, lg = self.forward(prompts)
        first = torch.stack([lg[b, lens[b] - 1] for b in range(B)])
        box = {"rows": rows}

        def step(tokens, parents):
            prev = box["rows"] if parents is None else [box["rows"][int(r)] for r in parents]
            box["rows"] = [torch.cat([p, self.E[int(t)][None]]) for p, t in zip(prev, tokens)]
            out = [self.forward(r[None]) for r in box["rows"]]
            return torch.stack([o[1][0, -1] for o in out]), torch.stack([o[0][0, -1] for o in out])

        return step, h, first

    def greedy(self, prompt, n):
        seq, ids = prompt, []
        for _ in range(n):
            t = int(self.forward(seq[None])[1][0, -1].argmax())
            ids.append(t)
            seq = torch.cat([seq, self.E[t][None]])
        return ids


def _prompts(B, S, d, seed):
    return torch.randn(B, S, d, generator=torch.Generator().manual_seed(seed))


def _run(toy, prompts, lengths, k, alpha, n, eos=-1, **kw):
    step, h, first = toy.driver(prompts, lengths, k)
    return contrastive_search(step, h, first, lengths, k, alpha, n, eos, **kw)


def test_top_k_one_is_greedy():
    toy, prompts = ToyLM(), _prompts(3, 5, 24, 1)
    toks, rec = _run(toy, prompts, None, 1, 0.6, 9)
    assert toks.tolist() == [toy.greedy(prompts[b], 9) for b in range(3)]
    assert contrastive_margin(rec) == math.inf and len(rec) == 9


def test_vanishing_alpha_is_greedy():
    toy, prompts = ToyLM(seed=3), _prompts(3, 5, 24, 2)
    alpha = 1e-6
    toks, rec = _run(toy, prompts, None, 4, alpha, 9)
    # decided: the two most probable candidates are further apart than the penalty term can move them (cosines span at most 2)
    assert all(float(((1 - alpha) * (r["p"][:, 0] - r["p"][:, 1])).min()) > 2 * alpha for r in rec)
    assert toks.tolist() == [toy.greedy(prompts[b], 9) for b in range(3)]


def test_contrastive_search_breaks_a_greedy_loop():
    toy, prompts = ToyLM(seed=6, copy=4.0), _prompts(2, 4, 24, 3)
    n = 12
    for b in range(2):
        g = toy.greedy(prompts[b], n)
        assert len(set(g[1:])) == 1, g                       # greedy decoding repeats one token for ever
    toks, rec = _run(toy, prompts, None, 4, 0.6, n)
    for row in toks.tolist():
        assert all(not (row[i] == row[i + 1] == row[i + 2]) for i in range(n - 2)), row
    assert math.isfinite(contrastive_margin(rec)) and contrastive_margin(rec) > 0


def test_ragged_rows_equal_rows_alone_and_padding_is_ignored():
    toy = ToyLM(seed=7)
    lengths = [6, 3, 4]
    prompts = _prompts(3, 6, 24, 4)
    toks, rec = _run(toy, prompts, lengths, 4, 0.6, 8)
    for b in range(3):
        alone, _ = _run(toy, prompts[b: b + 1, : lengths[b]], None, 4, 0.6, 8)
        assert toks[b].tolist() == alone[0].tolist()
    # hidden rows in the padding that would give cosine 1 with a candidate, were they looked at
    step, h, first = toy.driver(prompts, lengths, 4)
    h = h.clone()
    for b in range(3):
        h[b, lengths[b]:] = 1e3
    cand_h = []

    def spy(tokens, parents):
        lg, hid = step(tokens, parents)
        cand_h.append(hid)
        return lg, hid

    h[1, 3] = toy.forward(torch.cat([prompts[1, :3], toy.E[int(rec[0]["cand"][1, 0])][None]])[None])[0][0, -1]
    again, rec2 = contrastive_search(spy, h, first, lengths, 4, 0.6, 8, -1)
    assert torch.equal(again, toks)
    assert all(torch.equal(a["penalty"], b["penalty"]) for a, b in zip(rec, rec2))


def test_stop_on_eos_is_the_batch_wide_rule():
    toy, prompts = ToyLM(seed=9), _prompts(2, 4, 24, 5)
    toks, _ = _run(toy, prompts, None, 3, 0.6, 10)
    eos = int(toks[0, 2])
    hit = [i for i in range(10) if bool((toks[:, i] == eos).all())]
    cut, _ = _run(toy, prompts, None, 3, 0.6, 10, eos=eos)
    assert cut.shape[1] == (hit[0] + 1 if hit else 10) and torch.equal(cut, toks[:, : cut.shape[1]])
    full, _ = _run(toy, prompts, None, 3, 0.6, 10, eos=eos, stop_on_eos=False)
    assert torch.equal(full, toks)


# ------------------------------------------------------------------------------------------------- generate() on an LM object
class _HostLM:
    """An LM object without device token selection: its 'cache' is the embedded prefix, a (rows, T, d) tensor."""

    def __init__(self, toy):
        self.toy = toy
        self.config = SimpleNamespace(vocab_size=toy.V, head_rows=None)

    def __call__(self, input_ids=None, inputs_embeds=None, past_key_values=None, output_hidden_states=False, **kw):
        e = inputs_embeds if input_ids is None else torch.cat([past_key_values, self.toy.E[input_ids[:, 0]][:, None]], 1)
        h, lg = self.toy.forward(e)
        if input_ids is not None:
            h, lg = h[:, -1:], lg[:, -1:]
        return SimpleNamespace(logits=lg, hidden_states=[None, h], past_key_values=e)


class _HostModel(torch.nn.Module):
    def __init__(self, toy):
        super().__init__()
        self.lm, self.eos_token, self.image_token = _HostLM(toy), 1, 0


def test_generate_runs_the_host_statement_on_other_lm_objects():
    toy, prompts = ToyLM(seed=11), _prompts(2, 5, 24, 6)
    model = _HostModel(toy)
    out = generate(model, prompts, max_steps=7, penalty_alpha=0.6, top_k=4, decode=False, stop_on_eos=False)
    ref, _ = _run(toy, prompts, None, 4, 0.6, 7)
    assert out.shape == (2, 12) and torch.equal(out[:, 5:], ref) and bool((out[:, :5] == 0).all())


# --------------------------------------------------------------------------------------------------------------- the arguments
def test_check_contrastive_args():
    assert check_contrastive_args() is None and check_contrastive_args(0.0, 50) is None and check_contrastive_args(0, 0) is None
    assert check_contrastive_args(0.6, 4, 100) == (4, 0.6) and check_contrastive_args(1, 16) == (16, 1.0)
    for alpha in (float("nan"), float("inf"), -0.1, 1.5, True, "0.6", None):
        with pytest.raises(ValueError):
            check_contrastive_args(alpha, 4)
    with pytest.raises(ValueError, match="top_k in"):
        check_contrastive_args(0.6, 0)
    for k in (-1, 17, 4.0, True, None):
        with pytest.raises(ValueError):
            check_contrastive_args(0.6, k)
    with pytest.raises(ValueError, match="vocabulary"):
        check_contrastive_args(0.6, 8, vocab=5)


def test_generate_refuses_what_contrastive_search_is_not_combined_with():
    model = _HostModel(ToyLM())
    emb = _prompts(2, 4, 24, 0)
    kw = dict(penalty_alpha=0.6, top_k=4, max_steps=3)
    for more in (dict(num_beams=2), dict(return_scores=True), dict(repetition_penalty=1.2), dict(min_new_tokens=2),
                 dict(stop_per_row=True), dict(eos_token=[1, 2]), dict(stop_sequences=[[3, 4]]), dict(return_finish=True),
                 dict(return_logprobs=True), dict(constraint=[[3, 4]]),
                 dict(guidance_scale=2.0, negative_embeddings=_prompts(2, 3, 24, 1)), dict(past_key_values=object()),
                 dict(return_past_key_values=True)):
        with pytest.raises(NotImplementedError, match="contrastive"):
            generate(model, emb, **kw, **more)
    for bad in (dict(penalty_alpha=0.6), dict(penalty_alpha=0.6, top_k=17), dict(penalty_alpha=1.2, top_k=4),
                dict(penalty_alpha=float("nan"), top_k=4), dict(penalty_alpha=0.6, top_k=True),
                dict(penalty_alpha=0.6, top_k=41), dict(penalty_alpha=0.6, top_k=4, min_p=0.1, sampler="transformers")):
        with pytest.raises(ValueError):
            generate(model, emb, max_steps=3, **bad)


def test_selection_plan_mode_keys_and_refusals():
    from magma_amd.engine import LMEngine
    plain = LMEngine.selection_plan(vocab=100)
    assert LMEngine.selection_plan(vocab=100, contrast=None).keys == plain.keys       # penalty_alpha = 0: the greedy plan
    a = LMEngine.selection_plan(contrast=(4, 0.6), vocab=100)
    assert a.mode == ("contrast", 4, 0.6) and a.is_contrast and not a.is_beam and a.keys != plain.keys
    assert all(key.contrast and not key.beam for key in a.keys) and not any(key.contrast for key in plain.keys)
    assert a.keys != LMEngine.selection_plan(contrast=(5, 0.6), vocab=100).keys          # k and alpha are launch arguments
    assert a.keys != LMEngine.selection_plan(contrast=(4, 0.5), vocab=100).keys
    assert a.keys == LMEngine.selection_plan(contrast=(4, 0.6), vocab=100).keys
    assert len(a) == len(plain) and a._fields == plain._fields
    for more in (dict(beam=(2, 1.0, False, 4)), dict(processors=dict(repetition_penalty=1.2)), dict(stop=dict(eos_ids=[1, 2])),
                 dict(logprobs=0), dict(guidance=(2.0, 0.0))):
        with pytest.raises(NotImplementedError, match="contrastive"):
            LMEngine.selection_plan(contrast=(4, 0.6), vocab=100, **more)
    with pytest.raises(ValueError):
        LMEngine.selection_plan(contrast=(4, 0.6), sampling=(0.7, 0, 0.9), vocab=100)
    with pytest.raises(ValueError):
        LMEngine.selection_plan(contrast=(0, 0.6), vocab=100)
    with pytest.raises(ValueError):
        LMEngine.selection_plan(contrast=(8, 0.6), vocab=5)
