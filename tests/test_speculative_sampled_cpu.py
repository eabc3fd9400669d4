"""Speculative decoding for sampled rows and stop sequences, on the host (DESIGN.md "Speculative decoding"): the bookkeeping
statement speculate_update(stop_seqs=...) against stop_update applied after every single emitted token, the host loop over a tiny
GPT-J with stop sequences against the plain call, the engine's plan in the mode ("rows", warp), and the refusals that stay.
No GPU: test_spec_sampled_kernels_gpu.py runs the same cases (``CASES``, ``run_case``) through mg_spec_finish_seq."""
import pytest
import torch

from magma_amd.sampling import generate, speculate_update, stop_update
from test_beam_search_cpu import EOS, V, _tiny_gptj
from test_logits_processors_cpu import _HostMagma

I32, I64 = torch.int32, torch.int64
STOP_LEN = 0x300
VOCAB, COLS, POISON = 6, 24, -7


# ------------------------------------------------------------------------------------------------------------- the bookkeeping
def host_update(st, token, arm, kw):
    speculate_update(st["ids"], st["n_draft"], token, st["history"], st["count"], st["finish"], st["pos"], st["stats"], st["lookup"],
                     st["lookup_len"], st["state"], arm=arm, **kw)


def run_case(case, update=host_update, device="cpu"):
    """A speculative loop over ``case``: a model whose row b emits the fixed stream case["true"][b] -- fed row t of a step answers
    true[b][count + t] when the drafts in front of it were right and a wrong token otherwise (the bookkeeping never reads that
    one) --, the arming call, then steps until no row is open.  ``update(st, token, arm, kw)`` is the bookkeeping under test.
    Returns per row (kept tokens, count, finish record)."""
    true, T, lookup = case["true"], case["T"], case["lookup"]
    B, width = len(true), max(1, max(len(q) for q in lookup))
    z = lambda *s, dt=I32: torch.zeros(*s, dtype=dt, device=device)  # noqa: E731
    st = dict(ids=z(B, T, dt=I64), n_draft=z(B), history=torch.full((B, COLS), POISON, dtype=I64, device=device), count=z(B),
              finish=torch.tensor([[-1, 0]] * B, dtype=I32, device=device), pos=z(B), stats=z(B, 3), lookup=z(B, width),
              lookup_len=torch.tensor([len(q) for q in lookup], dtype=I32, device=device),
              state=torch.tensor([0, -1], dtype=I32, device=device))
    for b, q in enumerate(lookup):
        st["lookup"][b, :len(q)] = torch.tensor(q, dtype=I32)
    kw = dict(num_tokens=T - 1, max_ngram=case.get("max_ngram", 2), eos_ids=case["eos"], limit=case["limit"], vocab=VOCAB,
              stop_seqs=case["stop"])
    update(st, torch.tensor([r[0] for r in true], dtype=I64, device=device), True, kw)
    for _ in range(COLS + 2):
        if int(st["state"][1]) >= 0:
            break
        ids, count, fin = st["ids"].cpu(), st["count"].cpu(), st["finish"].cpu()
        token = torch.full((B * T,), VOCAB + 1, dtype=I64)               # rows the bookkeeping never reads: no token at all
        for b in range(B):
            if int(fin[b, 0]) >= 0:
                continue
            c = int(count[b])
            for t in range(int(st["n_draft"][b]) + 1):
                right = ids[b, 1:1 + t].tolist() == true[b][c:c + t]
                token[b * T + t] = true[b][c + t] if right else (true[b][c + t] + 1) % VOCAB
                if not right:
                    break
        update(st, token.to(device), False, kw)
    else:
        raise AssertionError("the loop never closed")
    hist, count, fin = st["history"].cpu(), st["count"].cpu(), st["finish"].cpu()
    assert all(hist[b, int(count[b]):].tolist() == [POISON] * (COLS - int(count[b])) for b in range(B)), "written past the count"
    return [(hist[b, :int(count[b])].tolist(), int(count[b]), tuple(fin[b].tolist())) for b in range(B)], st["stats"].cpu()


def token_by_token(case):
    """The rule the loop must equal: stop_update after every single token of the row's stream."""
    rows = []
    for r in case["true"]:
        hist, done, want = torch.tensor([r], dtype=I64), torch.tensor([False]), None
        for step in range(min(case["limit"], COLS)):
            done, reason = stop_update(hist, step, done, case["eos"], case["stop"])
            if bool(done[0]):
                want = (r[:step + 1], step + 1, (step + 1, (int(reason[0, 0]) << 8) | int(reason[0, 1])))
                break
        rows.append(want or (r[:min(case["limit"], COLS)], min(case["limit"], COLS), (min(case["limit"], COLS), STOP_LEN)))
    return rows


def _stream(g, n=COLS + 8):
    return torch.randint(0, VOCAB, (n,), generator=g).tolist()


def random_cases(B, T, n, seed):
    """Small random cases over a vocabulary of 6 (matches are frequent): eos id 5, stop sequences of length 1, 2 and 16, the
    row's own stream as lookup text (drafts are accepted), a random one (rejected) or none."""
    g = torch.Generator().manual_seed(seed)
    for i in range(n):
        true = [_stream(g) for _ in range(B)]
        for r in true:                      # (an eos id late in most rows: the sequences get their chance first)
            r[:6] = [t % 5 for t in r[:6]]
        stop = ([int(torch.randint(0, 5, (1,), generator=g))] if i % 3 == 0 else [], _stream(g, 2), _stream(g, 16))
        limit = int(torch.randint(1, COLS + 4, (1,), generator=g))
        if i % 4 == 0:                      # now and then row 0 lives long enough to complete a 16-token sequence, and does
            true[0] = [t % 5 for t in true[0]]
            stop, limit = ([], [], true[0][3:19]), COLS
        lookup = [[r, _stream(g), []][(i + b) % 3] for b, r in enumerate(true)]
        yield dict(name=f"random{B}x{T}-{i}", true=true, T=T, lookup=lookup, eos=(5,), stop=tuple(tuple(q) for q in stop if q),
                   limit=limit, max_ngram=1 + i % 3)


ROW = [1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3]
NAMED = [
    # arming emits 1; the lookup text continues 2 3 4 0: all four drafts are right, and token 4 (chunk row 2 of 5) ends [3, 4]
    dict(name="a draft completes a sequence in mid-chunk", true=[ROW], T=5, lookup=[ROW], eos=(5,), stop=((3, 4),), limit=20,
         want=[([1, 2, 3, 4], 4, (4, 0x200))]),
    # no lookup text and nothing repeats yet: one token per call, [2, 3] begins in one call and ends in the next
    dict(name="a sequence straddles two steps", true=[ROW], T=2, lookup=[[]], eos=(5,), stop=((2, 3),), limit=20,
         want=[([1, 2, 3], 3, (3, 0x200))]),
    dict(name="eos and a sequence on the same token: eos wins", true=[ROW], T=5, lookup=[ROW], eos=(5, 4), stop=((3, 4), (4,)),
         limit=20, want=[([1, 2, 3, 4], 4, (4, 0x100 | 1))]),
    # after one and two tokens every sequence is longer than the row: none may be compared (there is no column in front of the row's)
    dict(name="a sequence longer than the tokens emitted so far", true=[ROW], T=4, lookup=[ROW], eos=(5,),
         stop=((0, 1, 2), (POISON, 1), (4, 0, 1, 2)), limit=20, want=[([1, 2, 3, 4, 0, 1, 2], 7, (7, 0x200))]),
    dict(name="the lowest matching index wins", true=[ROW], T=8, lookup=[ROW], eos=(5,), stop=((9,), (2, 3), (3,)), limit=20,
         want=[([1, 2, 3], 3, (3, 0x200 | 1))]),
    dict(name="rows are independent", true=[ROW, ROW[2:] + [0, 1], ROW], T=4, lookup=[ROW, [], ROW], eos=(0,), stop=((2, 3),), limit=3,
         want=[([1, 2, 3], 3, (3, 0x200)), ([3, 4, 0], 3, (3, 0x100)), ([1, 2, 3], 3, (3, 0x200))]),
]
SHAPES = [(1, 2), (2, 8), (4, 4), (3, 5)]
CASES = NAMED + [c for B, T in SHAPES for c in random_cases(B, T, 12, seed=B * 10 + T)]


@pytest.mark.parametrize("case", NAMED, ids=lambda c: c["name"])
def test_named_cases(case):
    got, stats = run_case(case)
    assert got == case["want"] == token_by_token(case)
    if "draft completes" in case["name"]:
        assert stats[0].tolist() == [2, 4, 4], "the finishing token was meant to be an accepted draft"


def test_update_with_stop_sequences_is_stop_update_after_every_token():
    seen = {"stop": 0, "eos": 0, "length": 0, "accepted": 0, "long": 0}
    for case in CASES[len(NAMED):]:
        got, stats = run_case(case)
        want = token_by_token(case)
        assert got == want, (case, got, want)
        for (_, _, (_, code)), st in zip(got, stats.tolist()):
            seen[{1: "eos", 2: "stop", 3: "length"}[code >> 8]] += 1
            seen["accepted"] += st[2]
            seen["long"] += code >> 8 == 2 and len(case["stop"][code & 255]) == 16
    assert min(seen.values()) > 0 and seen["stop"] >= 20, seen
    assert {T for _, T in SHAPES} >= {2, 5, 8}


def test_without_stop_sequences_nothing_changed():
    for case in CASES[::5]:
        bare = dict(case, stop=())
        got, _ = run_case(bare)
        old, _ = run_case(bare, lambda st, token, arm, kw: host_update(st, token, arm, {k: v for k, v in kw.items() if k != "stop_seqs"}))
        assert got == old == token_by_token(bare)


# --------------------------------------------------------------------------------------------------------------- the host loop
@pytest.fixture(scope="module")
def tiny():
    return _tiny_gptj(seed=4, eos_bias=1.5), torch.randn(3, 5, 32, generator=torch.Generator().manual_seed(11))


def test_host_loop_with_stop_sequences_is_the_plain_call(tiny):
    """The host statement of the whole loop with stop sequences, on the toy LM, against the plain call with the same sequences:
    tokens and return_finish.  generate() itself keeps refusing this combination for an LM object without the engine (the next
    tests), so the loop behind it is called as generate() calls it on the engine."""
    from magma_amd.sampling import _generate_speculative, check_speculation_args
    lm, emb = tiny
    model = _HostMagma(lm)
    kw = dict(max_steps=12, temperature=0.0, decode=False, eos_token=[EOS, 3], return_finish=True)
    stopped = 0
    for r in range(emb.shape[0]):                   # (this LM keeps no per-row positions: row by row)
        free, _ = generate(model, emb[r:r + 1], **kw)
        toks = free[0, 5:].tolist()
        for seqs in ([toks[1:3]], [[V - 1, V - 3], toks[2:5], toks[0:1]], [toks[3:4]]):
            want, fin = generate(model, emb[r:r + 1], stop_sequences=seqs, **kw)
            for lookup in (None, [toks]):
                spec = check_speculation_args(3, 2, lookup, True, batch=1, vocab=V)
                got, fin2, sp = _generate_speculative(model, emb[r:r + 1], None, 12, (EOS, 3), False, None, True, spec, lookup, True, True,
                                                      tuple(tuple(q) for q in seqs))
                assert torch.equal(got, want), (r, seqs, got, want)
                assert torch.equal(fin2.kept, fin.kept) and fin2.reason == fin.reason and fin2.index == fin.index, (fin, fin2)
                stopped += fin2.reason[0] == "stop"
                if lookup is not None and int(fin.kept[0]) > 2:
                    assert int(sp.accepted[0]) > 0 and int(sp.steps[0]) < int(fin.kept[0])
    assert stopped >= 6, "no row stopped on a sequence: the test shows nothing"


# --------------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("warp", [False, True])
def test_engine_plan_takes_rows_mode_and_stop_sequences(warp):
    from magma_amd.engine import LMEngine
    stop = dict(eos_ids=(EOS,), stop_seqs=())
    seqs = dict(eos_ids=(EOS,), stop_seqs=((1, 2), (3,)))
    greedy = LMEngine.selection_plan(stop=stop, speculate=(4, 2), vocab=V)
    rows = LMEngine.selection_plan(stop=stop, speculate=(4, 2), sampling=("rows", warp), vocab=V)
    both = LMEngine.selection_plan(stop=seqs, speculate=(4, 2), sampling=("rows", warp), vocab=V)
    assert greedy.mode == ("speculate", 4, 2) and greedy.spec_rows is None
    assert greedy.spec_launches == ("mg_argmax_f32", "mg_spec_finish")
    assert rows.is_speculate and not rows.is_rows and rows.mode == ("speculate", 4, 2, ("rows", warp)) and rows.spec_rows is warp
    assert rows.spec_launches == ("mg_sample_chunk_f32", "mg_spec_finish")
    assert both.stop == ((EOS,), ((1, 2), (3,))) and both.spec_launches == ("mg_sample_chunk_f32", "mg_spec_finish_seq")
    with pytest.raises(NotImplementedError, match="rows"):          # the argmax plan keeps its two launches: stop sequences ride ("rows", warp)
        LMEngine.selection_plan(stop=seqs, speculate=(4, 2), vocab=V)
    keys = {p.graph_key(True) for p in (greedy, rows, both, LMEngine.selection_plan(stop=stop, speculate=(4, 2), vocab=V,
                                                                                   sampling=("rows", not warp)))}
    assert len(keys) == 4                           # the selection launch and the sequence count are launch arguments
    # another call's settings are table contents: nothing of them is in the plan
    assert rows == LMEngine.selection_plan(stop=stop, speculate=(4, 2), sampling=("rows", warp), vocab=V)
    for flat in ((0.7, 0, 0.9), ("warp", 0.7, 0, 0.9, 0.1)):
        with pytest.raises(NotImplementedError, match="rows"):
            LMEngine.selection_plan(stop=stop, speculate=(4, 2), sampling=flat, vocab=V)
    with pytest.raises(ValueError):
        LMEngine.selection_plan(stop=stop, speculate=(4, 2), sampling=("rows",), vocab=V)


# ----------------------------------------------------------------------------------------------------------------- the refusals
def test_a_host_lm_refuses_sampled_speculation(tiny):
    lm, emb = tiny
    model = _HostMagma(lm)
    kw = dict(max_steps=4, decode=False, prompt_lookup_num_tokens=2)
    for more in (dict(temperature=0.7), dict(), dict(temperature=0.7, seed=3, sampler="transformers", min_p=0.1),
                 dict(temperature=[0.0, 0.7, 0.0]), dict(temperature=0.0, seed=[1, 2, 3]),
                 dict(temperature=0.0, stop_sequences=[[1, 2]]), dict(stop_sequences=[[1, 2]])):
        with pytest.raises(ValueError, match="HIP engine") as e:
            generate(model, emb, **dict(kw, **more))
        assert isinstance(e.value, NotImplementedError)              # both: not implemented for this LM, and a value it cannot take
    with pytest.raises(ValueError, match="min_p.*HIP engine"):
        generate(model, emb, temperature=[0.0, 0.7, 0.7], min_p=0.1, sampler="transformers", **kw)
    with pytest.raises(ValueError, match="3 rows"):                       # the argument checks come first
        generate(model, emb, temperature=[0.7, 0.7], **kw)


def test_what_stays_refused(tiny):
    from magma_amd.sampling import TokenTrie, choose_stream, generate_stream
    lm, emb = tiny
    model = _HostMagma(lm)
    kw = dict(max_steps=4, decode=False, prompt_lookup_num_tokens=2)
    for t in (0.0, 0.7):
        for more in (dict(num_beams=2), dict(return_scores=True), dict(penalty_alpha=0.6, top_k=2),
                     dict(guidance_scale=1.5, negative_embeddings=emb), dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2),
                     dict(min_new_tokens=1), dict(suppress_tokens=[1]), dict(return_logprobs=True), dict(constraint=TokenTrie([[1, 2]])),
                     dict(return_past_key_values=True)):
            with pytest.raises(NotImplementedError):
                generate(model, emb, temperature=t, **dict(kw, **more))
        with pytest.raises(NotImplementedError, match="16"):
            generate(model, emb, temperature=t, max_steps=4, decode=False, prompt_lookup_num_tokens=7)
    with pytest.raises(NotImplementedError, match="speculative"):
        generate_stream(model, [emb[:1]], prompt_lookup_num_tokens=2, temperature=0.7)
    with pytest.raises(NotImplementedError, match="speculative"):
        choose_stream(model, [(emb[:1], [[1, 2]])], prompt_lookup_num_tokens=2)


def test_header_and_bindings_name_the_new_entry_points():
    import pathlib
    import re
    from magma_amd import lib, ops
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "magma_hip.h").read_text()
    assert re.search(r"#define MG_ABI_VERSION 27\b", text)
    for name in ("mg_sample_chunk_f32", "mg_spec_finish_seq"):
        assert re.search(rf"\bint {name}\(", text) and name in lib.SYMBOLS
        start = text.index("entry point   ")
        assert name in text[start:text.index("*/", start)], name
    assert len(lib.SYMBOLS["mg_spec_finish_seq"][1]) == len(lib.SYMBOLS["mg_spec_finish"][1]) + 1
    assert callable(ops.sample_chunk)
