"""Speculative greedy decoding on the host (magma_amd.sampling; DESIGN.md "Speculative decoding"): the draft rule pinned against
the installed transformers' PromptLookupCandidateGenerator, the bookkeeping statement speculate_update case by case, the host
loop over a tiny GPT-J against the per-row greedy call, every argument check and refusal, and the header's new entry points.
No GPU: the kernels and the engine's loop are compared with these statements in test_spec_kernels_gpu.py / test_speculative_gpu.py."""
import pathlib
import re

import pytest
import torch

from magma_amd.sampling import (Speculation, check_speculation_args, crop_past, generate, prompt_lookup, speculate_update)
from test_beam_search_cpu import EOS, V, _tiny_gptj
from test_logits_processors_cpu import _HostMagma

I32, I64 = torch.int32, torch.int64
STOP_EOS, STOP_LEN = 0x100, 0x300
TABLE = (([5, 6, 7, 8, 5, 6], [7, 8, 5]), ([7, 7, 7, 7], [7, 7]), ([5, 6, 9, 5, 6, 8, 5, 6], [9, 5, 6]), ([1, 2, 3, 4], []))


# ------------------------------------------------------------------------------------------------------------- the draft rule
def _hf_draft(ids, k, n, eos_ids):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(eos_token_id=torch.tensor(eos_ids) if eos_ids else None, num_output_tokens=k,
                                         max_matching_ngram_size=n, max_length=10 ** 6)
    x = torch.tensor([ids])
    return gen.get_candidates(x)[0][0, len(ids):].tolist()


@pytest.mark.parametrize("ids,draft", TABLE)
def test_prompt_lookup_examples(ids, draft):
    assert prompt_lookup(ids, 3, 2) == draft == _hf_draft(ids, 3, 2, ())


def test_prompt_lookup_is_transformers_rule():
    """A few hundred random sequences over a vocabulary of 6 (matches are common): lengths 2 to 40, 1 to 7 drafts, n-grams of 1 to
    4, with and without eos ids -- an eos id cuts the draft in front of it, and an emptied draft is no draft."""
    g = torch.Generator().manual_seed(0)
    seen = {"draft": 0, "none": 0, "cut": 0}
    for case in range(400):
        L, k, n = (int(torch.randint(lo, hi + 1, (1,), generator=g)) for lo, hi in ((2, 40), (1, 7), (1, 4)))
        ids = torch.randint(0, 6, (L,), generator=g).tolist()
        eos_ids = ((), (5,), (0, 3))[case % 3]
        want = _hf_draft(ids, k, n, eos_ids)
        assert prompt_lookup(ids, k, n, eos_ids) == want, (ids, k, n, eos_ids)
        seen["draft" if want else "none"] += 1
        seen["cut"] += bool(eos_ids) and want != _hf_draft(ids, k, n, ())
    assert min(seen.values()) > 10, seen
    assert prompt_lookup([3], 3, 2) == [] and prompt_lookup([], 3, 2) == []
    assert prompt_lookup([1, 2, 9, 1, 2], 3, 2, vocab=6) == []          # an id outside the vocabulary cuts like an eos id


# ------------------------------------------------------------------------------------------------------------- the bookkeeping
T, COLS = 4, 16


def _state(ids, nd, token, hist, finish=(-1, 0), lookup=(), pos=40, step=3):
    h = torch.full((1, COLS), -7, dtype=I64)
    h[0, :len(hist)] = torch.tensor(hist, dtype=I64)
    lk = torch.full((1, 8), -7, dtype=I32)
    lk[0, :len(lookup)] = torch.tensor(lookup, dtype=I32)
    return dict(ids=torch.tensor([ids], dtype=I64), n_draft=torch.tensor([nd], dtype=I32), token=torch.tensor(token, dtype=I64),
                history=h, count=torch.tensor([len(hist)], dtype=I32), finish=torch.tensor([list(finish)], dtype=I32),
                pos=torch.tensor([pos], dtype=I32), stats=torch.zeros(1, 3, dtype=I32), lookup=lk,
                lookup_len=torch.tensor([len(lookup)], dtype=I32), state=torch.tensor([step, -1], dtype=I32))


def _update(st, limit=COLS, arm=False, num_tokens=3, max_ngram=2, eos_ids=(5,)):
    speculate_update(st["ids"], st["n_draft"], st["token"], st["history"], st["count"], st["finish"], st["pos"], st["stats"],
                     st["lookup"], st["lookup_len"], st["state"], num_tokens=num_tokens, max_ngram=max_ngram, eos_ids=eos_ids,
                     limit=limit, arm=arm, vocab=8)
    return st


def test_update_full_acceptance():
    w = _update(_state([1, 2, 3, 4], 3, [2, 3, 4, 1], [0, 1]))
    assert w["history"][0, :6].tolist() == [0, 1, 2, 3, 4, 1] and w["count"].tolist() == [6] and w["pos"].tolist() == [44]
    assert w["stats"].tolist() == [[1, 3, 3]] and w["finish"].tolist() == [[-1, 0]] and w["state"].tolist() == [4, -1]
    # the next drafts: the sequence 0 1 2 3 4 1 ends with "1"; its first occurrence is followed by 2 3 4
    assert w["ids"].tolist() == [[1, 2, 3, 4]] and w["n_draft"].tolist() == [3]
    assert w["history"][0, 6:].tolist() == [-7] * (COLS - 6)


def test_update_partial_acceptance():
    w = _update(_state([1, 2, 3, 4], 3, [2, 0, 4, 1], [0, 1]))           # the model says 0 where draft 2 said 3
    assert w["history"][0, :4].tolist() == [0, 1, 2, 0] and w["count"].tolist() == [4] and w["pos"].tolist() == [42]
    assert w["stats"].tolist() == [[1, 3, 1]]
    assert w["ids"][0, 0].item() == 0 and w["ids"].tolist() == [[0, 1, 2, 0]] and w["n_draft"].tolist() == [3]


def test_update_zero_acceptance_and_no_draft():
    w = _update(_state([1, 2, 3, 4], 3, [4, 3, 4, 1], [0, 1]))
    assert w["history"][0, :3].tolist() == [0, 1, 4] and w["count"].tolist() == [3] and w["pos"].tolist() == [41]
    assert w["stats"].tolist() == [[1, 3, 0]]
    assert w["ids"].tolist() == [[4, 4, 4, 4]] and w["n_draft"].tolist() == [0]      # unused entries repeat the last token


def test_update_eos_inside_the_accepted_run():
    w = _update(_state([1, 2, 5, 4], 3, [2, 5, 4, 1], [0, 1]))
    assert w["history"][0, :4].tolist() == [0, 1, 2, 5] and w["history"][0, 4].item() == -7          # the eos is kept, the rest cut
    assert w["count"].tolist() == [4] and w["finish"].tolist() == [[4, STOP_EOS | 0]]
    assert w["n_draft"].tolist() == [0] and w["ids"].tolist() == [[5] * T] and w["state"].tolist() == [4, 3]
    w = _update(_state([1, 2, 3, 4], 3, [2, 6, 4, 1], [0, 1]), eos_ids=(5, 6))                    # the model's own token is eos id 1
    assert w["count"].tolist() == [4] and w["finish"].tolist() == [[4, STOP_EOS | 1]]


def test_update_the_limit_cuts_the_run():
    w = _update(_state([1, 2, 3, 4], 3, [2, 3, 4, 1], [0, 1]), limit=4)
    assert w["history"][0, :4].tolist() == [0, 1, 2, 3] and w["history"][0, 4].item() == -7
    assert w["count"].tolist() == [4] and w["finish"].tolist() == [[4, STOP_LEN]] and w["state"].tolist() == [4, 3]
    w = _update(_state([1, 2, 3, 4], 3, [2, 3, 4, 1], [0, 1] * 7), limit=100)                     # the history's width bounds too
    assert w["count"].tolist() == [COLS] and w["finish"].tolist() == [[COLS, STOP_LEN]]


def test_update_a_finished_row_stays_frozen():
    st = _state([1, 2, 3, 4], 3, [2, 3, 4, 1], [0, 1], finish=(2, STOP_EOS))
    before = {k: v.clone() for k, v in st.items()}
    w = _update(st)
    for k in ("history", "count", "finish", "pos", "stats"):
        assert torch.equal(w[k], before[k]), k
    assert w["n_draft"].tolist() == [0] and w["ids"].tolist() == [[5] * T] and w["state"].tolist() == [4, 3]


def test_update_the_arming_call():
    w = _update(_state([0, 0, 0, 0], 0, [2], [], lookup=[1, 2, 3, 4, 1], step=0), arm=True)
    assert w["history"][0, 0].item() == 2 and w["count"].tolist() == [1] and w["pos"].tolist() == [40]      # nothing was fed
    assert w["ids"].tolist() == [[2, 3, 4, 1]] and w["n_draft"].tolist() == [3] and w["stats"].tolist() == [[1, 0, 0]]
    assert w["state"].tolist() == [1, -1]
    w = _update(_state([0, 0, 0, 0], 3, [5], [], step=0), arm=True)      # token 0 is an eos id; a stale n_draft counts as 0
    assert w["finish"].tolist() == [[1, STOP_EOS]] and w["state"].tolist() == [1, 0] and w["stats"].tolist() == [[1, 0, 0]]


def test_update_rows_are_independent_and_degenerate_values_are_clamped():
    a, b = _state([1, 2, 3, 4], 3, [2, 3, 4, 1], [0, 1]), _state([1, 2, 3, 4], 9, [2, 0, 4, 1], [0, 1])
    both = {k: torch.cat([a[k], b[k]]) for k in a if k != "state"}
    both["state"] = a["state"].clone()
    w = _update(both)
    assert w["count"].tolist() == [6, 4] and w["stats"].tolist() == [[1, 3, 3], [1, 3, 1]]       # n_draft 9 counts as T - 1
    st = _state([1, 2, 3, 4], 3, [2, 3, 4, 1], [0, 1])
    st["count"][0] = -2
    before = {k: v.clone() for k, v in st.items()}
    w = _update(st)
    assert all(torch.equal(w[k], before[k]) for k in st if k != "state") and w["state"].tolist() == [4, 3]
    st = _state([1, 2, 3, 4], 0, [2, 3, 4, 1], [0, 1], lookup=[6, 6, 7])
    st["lookup_len"][0] = 99                                             # counts as the buffer's 8 columns; the poison is no token
    assert _update(st)["n_draft"].tolist() == [0]


# --------------------------------------------------------------------------------------------------------------- the host loop
@pytest.fixture(scope="module")
def tiny():
    # seed 4: the greedy run repeats itself and reaches eos within a few steps (test_logits_processors_cpu)
    return _tiny_gptj(seed=4, eos_bias=1.5), torch.randn(3, 5, 32, generator=torch.Generator().manual_seed(11))


def _greedy_rows(model, emb, lens, **kw):
    """The per-row greedy call, every row alone with its own prompt (this LM keeps no per-row positions)."""
    rows = []
    for r in range(emb.shape[0]):
        out, fin = generate(model, emb[r:r + 1, :lens[r]], temperature=0.0, decode=False, stop_per_row=True, return_finish=True, **kw)
        rows.append((out[0, lens[r]:lens[r] + int(fin.kept[0])].tolist(), fin.reason[0]))
    return rows


@pytest.mark.parametrize("lens,k", [([5], 1), ([5], 3), ([5], 7), ([5, 2, 4], 1), ([5, 2, 4], 4)])
@pytest.mark.parametrize("lookup", ["none", "hit", "miss"])
def test_host_loop_is_the_greedy_call(tiny, lens, k, lookup):
    lm, emb = tiny
    model, emb = _HostMagma(lm), emb[:len(lens)]
    kw = dict(max_steps=12, eos_token=[EOS, 3])
    want = _greedy_rows(model, emb, lens, **kw)
    ids = {"none": None, "hit": [w[0] for w in want], "miss": [[V - 1, V - 3] * 3 for _ in lens]}[lookup]
    out, fin, sp = generate(model, emb, lengths=lens if len(lens) > 1 else None, temperature=0.0, decode=False, return_finish=True,
                            prompt_lookup_num_tokens=k, lookup_ids=ids, return_speculation=True, **kw)
    n = max(len(w[0]) for w in want)
    assert out.shape == (len(lens), emb.shape[1] + n) and isinstance(sp, Speculation)
    for r, (toks, reason) in enumerate(want):
        assert out[r, lens[r]:lens[r] + len(toks)].tolist() == toks and int(fin.kept[r]) == len(toks) and fin.reason[r] == reason
        assert out[r, :lens[r]].tolist() == [model.image_token] * lens[r]
        assert out[r, lens[r] + len(toks):].tolist() == [EOS] * (out.shape[1] - lens[r] - len(toks))
    assert (sp.accepted <= sp.drafted).all() and (sp.steps >= 1).all()
    if lookup == "hit":         # the answer itself is there to be looked up: every step but the prefill emits several tokens
        assert int(sp.accepted.sum()) > 0 and all(int(sp.steps[r]) <= len(w[0]) for r, w in enumerate(want))
        long = [r for r, w in enumerate(want) if len(w[0]) > 2]
        assert all(int(sp.steps[r]) < len(want[r][0]) for r in long)
    if lookup == "miss" and k == 1:
        assert int(sp.steps.max()) <= 12


def test_host_loop_fixed_width_and_text(tiny):
    lm, emb = tiny
    model = _HostMagma(lm)
    a = generate(model, emb[:1], max_steps=9, temperature=0.0, decode=False, stop_per_row=True, stop_on_eos=False)
    b = generate(model, emb[:1], max_steps=9, temperature=0.0, decode=False, stop_on_eos=False, prompt_lookup_num_tokens=3)
    assert torch.equal(a, b) and b.shape[1] == 5 + 9


def test_crop_past():
    t = torch.arange(2 * 3 * 6 * 4).view(2, 3, 6, 4)
    assert torch.equal(crop_past(((t, t + 1),), 4)[0][1], (t + 1)[:, :, :4])
    import transformers
    c = transformers.DynamicCache()
    c.update(t.float(), t.float(), 0)
    assert crop_past(c, 2).get_seq_length() == 2
    with pytest.raises(TypeError):
        crop_past(object(), 1)


# ------------------------------------------------------------------------------------------------------------------ the checks
def test_check_speculation_args():
    assert check_speculation_args() is None
    assert check_speculation_args(3, 2, [[1, 2], torch.tensor([3])], batch=2, vocab=9) == dict(T=4, max_ngram=2, lookup=[[1, 2], [3]])
    assert check_speculation_args(7, 16, ["ab"], encode=lambda q: [ord(c) for c in q])["lookup"] == [[97, 98]]
    for bad in (dict(prompt_lookup_num_tokens=8), dict(prompt_lookup_num_tokens=-1), dict(prompt_lookup_num_tokens=True),
                dict(prompt_lookup_num_tokens=2.0), dict(prompt_lookup_num_tokens=2, max_matching_ngram_size=0),
                dict(prompt_lookup_num_tokens=2, max_matching_ngram_size=17), dict(lookup_ids=[[1]]), dict(return_speculation=True),
                dict(prompt_lookup_num_tokens=2, lookup_ids="ab"), dict(prompt_lookup_num_tokens=2, lookup_ids=[[1]], batch=2),
                dict(prompt_lookup_num_tokens=2, lookup_ids=[[9]], vocab=9), dict(prompt_lookup_num_tokens=2, lookup_ids=[[-1]]),
                dict(prompt_lookup_num_tokens=2, lookup_ids=[[True]]), dict(prompt_lookup_num_tokens=2, lookup_ids=["ab"]),
                dict(prompt_lookup_num_tokens=2, lookup_ids=[3])):
        with pytest.raises(ValueError):
            check_speculation_args(**bad)
    with pytest.raises(NotImplementedError, match="16"):
        check_speculation_args(7, 2, batch=3)


def test_refusals(tiny):
    lm, emb = tiny
    model = _HostMagma(lm)
    kw = dict(max_steps=4, decode=False, prompt_lookup_num_tokens=2)
    from magma_amd.sampling import TokenTrie
    for more in (dict(temperature=0.7), dict(temperature=[0.0, 0.0, 0.0]), dict(temperature=0.0, num_beams=2),
                 dict(temperature=0.0, return_scores=True), dict(temperature=0.0, penalty_alpha=0.6, top_k=2),
                 dict(temperature=0.0, guidance_scale=1.5, negative_embeddings=emb), dict(temperature=0.0, repetition_penalty=1.2),
                 dict(temperature=0.0, no_repeat_ngram_size=2), dict(temperature=0.0, min_new_tokens=1),
                 dict(temperature=0.0, suppress_tokens=[1]), dict(temperature=0.0, return_logprobs=True),
                 dict(temperature=0.0, constraint=TokenTrie([[1, 2]])), dict(temperature=0.0, stop_sequences=[[1, 2]]),
                 dict(temperature=0.0, return_past_key_values=True)):
        with pytest.raises(NotImplementedError):
            generate(model, emb, **dict(kw, **more))
    with pytest.raises(NotImplementedError, match="16"):
        generate(model, emb, temperature=0.0, max_steps=4, decode=False, prompt_lookup_num_tokens=7)
    with pytest.raises(ValueError, match="stop_per_row"):
        generate(model, emb, temperature=0.0, stop_per_row=False, **kw)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        generate(model, emb, temperature=0.0, max_steps=4, decode=False, lookup_ids=[[1]] * 3)
    with pytest.raises(ValueError, match="eos_token"):
        generate(model, emb, temperature=0.0, eos_token=list(range(9)), **kw)


def test_stream_entry_points_refuse_speculation(tiny):
    from magma_amd.sampling import choose_stream, generate_stream
    lm, emb = tiny
    model = _HostMagma(lm)
    for kw in (dict(prompt_lookup_num_tokens=2), dict(lookup_ids=[[1]]), dict(return_speculation=True), dict(max_matching_ngram_size=3)):
        with pytest.raises(NotImplementedError, match="speculative"):
            generate_stream(model, [emb[:1]], **kw)
        with pytest.raises(NotImplementedError, match="speculative"):
            choose_stream(model, [(emb[:1], [[1, 2]])], **kw)
    with pytest.raises(TypeError):
        choose_stream(model, [(emb[:1], [[1, 2]])], no_such_keyword=1)


def test_engine_plan_refuses_what_speculation_is_not_combined_with():
    from magma_amd.engine import LMEngine
    stop = dict(eos_ids=(EOS,), stop_seqs=())
    plan = LMEngine.selection_plan(stop=stop, speculate=(4, 2), vocab=V)
    assert plan.is_speculate and plan.mode == ("speculate", 4, 2) and plan.stop == ((EOS,), ())
    assert plan.graph_key(True) != LMEngine.selection_plan(stop=stop, speculate=(4, 3), vocab=V).graph_key(True)
    assert not LMEngine.selection_plan(stop=stop, vocab=V).is_speculate
    for more in (dict(sampling=(0.7, 0, 0.9)), dict(beam=(2, 1.0, False, 8)), dict(processors=dict(repetition_penalty=1.2)),
                 dict(logprobs=0), dict(guidance=(1.5, 0.0)), dict(contrast=(2, 0.6)), dict(slots=True)):
        with pytest.raises(NotImplementedError):
            LMEngine.selection_plan(stop=stop, speculate=(4, 2), vocab=V, **more)
    with pytest.raises(NotImplementedError):
        LMEngine.selection_plan(speculate=(4, 2), vocab=V)
    with pytest.raises(NotImplementedError):
        LMEngine.selection_plan(stop=dict(eos_ids=(EOS,), stop_seqs=((1, 2),)), speculate=(4, 2), vocab=V)
    for bad in ((1, 2), (9, 2), (4, 0), (4, 17), (True, 2)):
        with pytest.raises(ValueError):
            LMEngine.selection_plan(stop=stop, speculate=bad, vocab=V)


def test_default_call_is_untouched(tiny):
    """prompt_lookup_num_tokens=0: generate() takes the branch it took (no speculative loop is entered)."""
    import magma_amd.sampling as S
    lm, emb = tiny
    model = _HostMagma(lm)
    want = generate(model, emb, max_steps=6, temperature=0.0, decode=False)
    entered = []
    orig = S._generate_speculative
    S._generate_speculative = lambda *a, **k: entered.append(1) or orig(*a, **k)
    try:
        got = generate(model, emb, max_steps=6, temperature=0.0, decode=False, prompt_lookup_num_tokens=0)
    finally:
        S._generate_speculative = orig
    assert torch.equal(got, want) and not entered


# ------------------------------------------------------------------------------------------------------------------ the header
def test_header_names_the_entry_points():
    from magma_amd import lib
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "magma_hip.h").read_text()
    assert re.search(r"#define MG_ABI_VERSION 27\b", text)
    for name in ("mg_attn_decode_chunk_bf16", "mg_decode_attn_gemv_chunk_bf16", "mg_spec_finish"):
        assert re.search(rf"\bint {name}\(", text) and name in lib.SYMBOLS
        start = text.index("entry point   ")                        # the table of "Device-resident indices"
        assert name in text[start:text.index("*/", start)], name
