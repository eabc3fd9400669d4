"""Speculative decoding for sampled rows and with stop sequences on the engine (DESIGN.md "Speculative decoding"), on the reduced
model of tests/test_continue_generate_gpu.py.

The mode is seed-exact by construction -- fed row t of sequence b is drawn at the Philox counter count[b] + t under b's record,
the counter and record of the plain per-row call's token count[b] + t -- so every comparison is an equality:
  * one sampled speculative step selects, for every fed row the bookkeeping reads, what ops.sample_rows selects on the logits of
    the plain step over B * T rows (the same bits: asserted) at that counter;
  * generate(prompt_lookup_num_tokens = T - 1) with sampled and greedy rows is token for token the plain per-row sampled call,
    whether the drafts are right (the lookup text is the answer) or wrong (random ids) -- under the asserted precondition that the
    prompts' plain greedy ids agree between the B-row and the B * T-row shapes;
  * with stop sequences, tokens, kept counts and reasons are the plain call's;
  * the step's launches are the greedy speculative step's with mg_argmax_f32 replaced by the chunk selection."""
import pytest
import torch

from test_continue_generate_gpu import embeds, model, oracle  # noqa: F401  (fixtures)
from test_speculative_gpu import LENS, padded, tokens

pytestmark = pytest.mark.gpu

STEPS = 14
SHAPES = [(1, 4), (2, 8), (3, 5)]
ROWS = {1: dict(temperature=[0.8], top_k=[40], seed=[11]),
        2: dict(temperature=[0.0, 0.8], top_k=[0, 40], seed=[11, 12]),
        3: dict(temperature=[0.9, 0.0, 1.1], top_k=[40, 0, 5], seed=[11, 12, 13])}
WARP = {1: dict(min_p=[0.02], top_p=[0.95]), 2: dict(min_p=[0.0, 0.02], top_p=[0.9, 0.95]),
        3: dict(min_p=[0.02, 0.0, 0.0], top_p=[0.95, 0.9, 0.5])}


def run(m, emb, lens, steps=STEPS, **kw):
    from magma_amd.sampling import generate
    return generate(m, emb, lengths=lens, max_steps=steps, decode=False, **kw)


def prompts_of(m, B, T):
    """B ragged prompts whose plain greedy ids agree between the B-row call and the B * T-row call on the prompts repeated: the
    precondition of comparing a step over B * T rows with steps over B rows (the claim is about the selection, not GEMV shapes)."""
    emb, lens = padded(m, embeds(m, LENS[:B], seed=22))
    g = tokens(run(m, emb, lens, temperature=0.0, eos_token=-7), lens, STEPS)
    wide_lens = [n for n in lens for _ in range(T)]
    wide = tokens(run(m, emb.repeat_interleave(T, 0), wide_lens, temperature=0.0, eos_token=-7), wide_lens, STEPS)
    assert wide == [r for r in g for _ in range(T)], "pick other prompts: these decode differently at B and at B * T rows already"
    return emb, lens, g


def settings(B, sampler):
    return dict(ROWS[B], **(WARP[B] if sampler == "transformers" else {}), sampler=sampler)


def same_finish(a, b):
    return torch.equal(a.kept, b.kept) and a.reason == b.reason and a.index == b.index


# ---------------------------------------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("warp", [False, True])
@pytest.mark.parametrize("B,T", SHAPES)
def test_one_sampled_speculative_step_selects_what_sample_rows_selects_on_the_plain_steps_logits(model, B, T, warp):  # noqa: F811
    from magma_amd import ops
    from magma_amd.engine import LMEngine
    from magma_amd.sampling import check_row_sampler_args
    eng, dev = model.lm.engine, model.device
    emb, lens = padded(model, embeds(model, LENS[:B], seed=31))
    kw = settings(B, "transformers" if warp else "reference")
    table = ops.sample_rows_table(*zip(*check_row_sampler_args(B, **kw)))
    free = eng.V - 1
    plan = LMEngine.selection_plan(stop=dict(eos_ids=(free,), stop_seqs=()), speculate=(T, 4), sampling=("rows", warp), vocab=eng.V)
    answer = tokens(run(model, emb, lens, eos_token=[free], stop_per_row=True, **kw), lens, STEPS)
    assert all(free not in r for r in answer), "pick another eos id: the sampled rows emit this one"
    with torch.no_grad():
        out = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=STEPS + T, eos_token=free, plan=plan, lengths=lens,
                       seed=dict(limit=STEPS, lookup=answer, rows=table))
        cache = out.past_key_values
        st = cache.spec[T]
        ids, count, nd = st.ids.view(B, T).clone(), st.count.tolist(), st.n_draft.tolist()
        assert count == [1] * B and [int(ids[b, 0]) for b in range(B)] == [r[0] for r in answer]       # token 0: the arming call's draw
        assert max(nd) > 0, "no drafts: the answer was there to be looked up"
        # the plain statement of the step's logits (tests/test_speculative_gpu.py): row b * T + t holds prompt b and ids[b, :t]
        lens_r = torch.tensor(lens).repeat_interleave(T)
        _, narrow, _ = eng.prefill(emb, cache_hint=T + 8, lengths=torch.tensor(lens))
        wide = narrow.expand(T)
        t_of = torch.arange(T).repeat(B)
        for j in range(T - 1):
            eng.decode(ids[:, j].repeat_interleave(T).view(B * T, 1), wide, use_graph=False, select=False)
            wide.set_rows(lens_r + torch.minimum(t_of, torch.tensor(j + 1)))
        want_logits, _ = eng.decode(ids.reshape(B * T, 1), wide, use_graph=False, select=False)
        want_logits = want_logits.clone()
        got_logits, got = eng.decode(None, cache, use_graph=False, plan=plan)
        got_logits, got = got_logits.clone(), got.clone()
        torch.cuda.synchronize()
        assert torch.equal(got_logits, want_logits), "the step's logits are not the plain step's over B * T rows"
        tab = table.to(dev)
        for b in range(B):
            for t in range(nd[b] + 1):
                state = torch.tensor([count[b] + t, -1], dtype=torch.int32, device=dev)
                want = ops.sample_rows(want_logits[b * T + t: b * T + t + 1], tab[b:b + 1], state, warp)
                assert int(got[b * T + t]) == int(want[0]), (b, t, int(got[b * T + t]), int(want[0]))


# -------------------------------------------------------------------------------------------------------------------- whole calls
def sampled_cases(m, B, T, sampler):
    emb, lens, greedy = prompts_of(m, B, T)
    free = m.lm.engine.V - 1
    kw = dict(settings(B, sampler), eos_token=[free], stop_per_row=True, return_finish=True)
    want, fin = run(m, emb, lens, **kw)
    rows = tokens(want, lens, STEPS)
    assert all(free not in r for r in rows), "pick another eos id: the sampled rows emit this one"
    drawn = [b for b, t in enumerate(kw["temperature"]) if t > 0.0]
    assert all(rows[b] == greedy[b] for b in range(B) if b not in drawn)        # a greedy row is the greedy call's
    assert any(rows[b] != greedy[b] for b in drawn), "the sampled rows repeat the greedy ids: nothing is drawn"
    g = torch.Generator().manual_seed(B * 10 + T)
    noise = [torch.randint(0, free, (40,), generator=g).tolist() for _ in range(B)]
    for name, lookup in (("itself", rows), ("random", noise)):
        got, fin2, sp = run(m, emb, lens, prompt_lookup_num_tokens=T - 1, max_matching_ngram_size=8, lookup_ids=lookup,
                            return_speculation=True, **kw)
        what = f"B={B} T={T} {sampler} lookup={name}"
        assert torch.equal(got, want), f"{what}: {tokens(got, lens, STEPS)} != {rows}"
        assert same_finish(fin2, fin), what
        assert bool((sp.accepted <= sp.drafted).all()) and bool((sp.steps >= 1).all()), what
        if name == "itself":
            assert int(sp.accepted.min()) > 0 and int(sp.steps.max()) < STEPS, (what, sp)     # fewer steps than tokens
    return emb, lens, kw, want


@pytest.mark.parametrize("sampler", ["reference", "transformers"])
@pytest.mark.parametrize("B,T", SHAPES)
def test_generate_is_the_plain_per_row_sampled_call_token_for_token(model, B, T, sampler):  # noqa: F811
    sampled_cases(model, B, T, sampler)


def test_scalar_settings_stand_for_every_row_and_seeds_are_the_rows_own(model):  # noqa: F811
    B, T = 2, 4
    emb, lens, _ = prompts_of(model, B, T)
    free = model.lm.engine.V - 1
    kw = dict(eos_token=[free], prompt_lookup_num_tokens=T - 1)
    scalar = run(model, emb, lens, temperature=0.8, top_k=40, seed=5, **kw)
    per_row = run(model, emb, lens, temperature=[0.8, 0.8], top_k=[40, 40], seed=[5, 5], **kw)
    plain = run(model, emb, lens, temperature=[0.8, 0.8], top_k=[40, 40], seed=[5, 5], eos_token=[free], stop_per_row=True)
    assert torch.equal(scalar, per_row) and torch.equal(scalar, plain)
    assert torch.equal(run(model, emb, lens, temperature=0.8, top_k=40, seed=5, **kw), scalar)          # a repeated call reproduces
    other = tokens(run(model, emb, lens, temperature=0.8, top_k=40, seed=[5, 6], **kw), lens, STEPS)
    rows = tokens(scalar, lens, STEPS)
    assert other[0] == rows[0] and other[1] != rows[1]                  # another seed for row 1 changes row 1 alone
    for b in range(B):                                                  # row b is generate(row_b, seed=s_b) alone
        alone = run(model, emb[b:b + 1], lens[b:b + 1], temperature=0.8, top_k=40, seed=[5, 6][b], eos_token=[free], stop_per_row=True)
        assert tokens(alone, lens[b:b + 1], STEPS)[0] == other[b], b
    unseeded = [tokens(run(model, emb, lens, temperature=0.8, top_k=40, **kw), lens, STEPS) for _ in range(2)]
    assert unseeded[0] != unseeded[1]                                   # seed=None draws seeds of its own


# ------------------------------------------------------------------------------------------------------------------ stop sequences
@pytest.mark.parametrize("sampled", [True, False])
def test_stop_sequences_complete_inside_accepted_drafts(model, sampled):  # noqa: F811
    B, T = 2, 4
    emb, lens, _ = prompts_of(model, B, T)
    free = model.lm.engine.V - 1
    how = dict(temperature=[0.8, 0.9], top_k=[40, 40], seed=[21, 22]) if sampled else dict(temperature=0.0)
    base = dict(how, eos_token=[free], stop_per_row=True, return_finish=True)
    rows = tokens(run(model, emb, lens, **base)[0], lens, STEPS)
    # from the plain call's own output, so they are certain to fire: row 0's tokens 6..7, row 1's token 9 and (never) a long one
    seqs = [rows[0][6:8], rows[1][9:10], rows[0][:4] + [free - 1] * 12]
    want, fin = run(model, emb, lens, stop_sequences=seqs, **base)
    assert "stop" in fin.reason and int(fin.kept.min()) < STEPS, fin
    got, fin2, sp = run(model, emb, lens, stop_sequences=seqs, prompt_lookup_num_tokens=T - 1, max_matching_ngram_size=8,
                        lookup_ids=rows, return_speculation=True, **base)
    assert torch.equal(got, want), (tokens(got, lens, STEPS), tokens(want, lens, STEPS))
    assert same_finish(fin2, fin) and "stop" in fin2.reason, (fin, fin2)
    stopped = [b for b in range(B) if fin2.reason[b] == "stop"]
    # fewer model calls than tokens in a stopped row: its finishing token came inside a run of accepted drafts or right behind it
    assert any(int(sp.accepted[b]) > 0 and int(sp.steps[b]) < int(fin2.kept[b]) for b in stopped), (fin2, sp)
    none, fin3 = run(model, emb, lens, stop_sequences=seqs, prompt_lookup_num_tokens=T - 1, **base)      # and with nothing to look up
    assert torch.equal(none, want) and same_finish(fin3, fin)


# -------------------------------------------------------------------------------------------------------------------- the launches
def step_records(eng, cache, plan, T):
    import launch_trace as lt
    held, cache.decode_state = cache.decode_state, cache.spec[T]
    try:
        recs, res = lt.record(eng, lambda: eng.decode(None, cache, use_graph=False, plan=plan), cache=cache,
                              op_names=lt.OPS + ("attn_decode_chunk", "spec_finish", "sample_chunk", "sample_rows"))
    finally:
        cache.decode_state = held
    if isinstance(res, Exception):
        raise res
    return recs


@pytest.mark.parametrize("T", [4, 8])
def test_the_sampled_step_is_the_greedy_speculative_step_with_the_selection_replaced(model, T):  # noqa: F811
    from magma_amd import ops
    from magma_amd.engine import LMEngine
    from magma_amd.sampling import check_row_sampler_args
    eng, B = model.lm.engine, 2
    emb, lens = padded(model, embeds(model, LENS[:B], seed=22))
    stop = dict(eos_ids=(model.eos_token,), stop_seqs=())
    greedy = LMEngine.selection_plan(stop=stop, speculate=(T, 2), vocab=eng.V)
    rows = LMEngine.selection_plan(stop=stop, speculate=(T, 2), sampling=("rows", False), vocab=eng.V)
    table = ops.sample_rows_table(*zip(*check_row_sampler_args(B, **ROWS[B])))
    kw = dict(inputs_embeds=emb, use_cache=True, cache_hint=STEPS + T, eos_token=model.eos_token, lengths=lens)
    with torch.no_grad():
        out = model.lm(plan=greedy, seed=dict(limit=STEPS, lookup=None), **kw)
        a = step_records(eng, out.past_key_values, greedy, T)
        out = model.lm(plan=rows, seed=dict(limit=STEPS, lookup=None, rows=table), **kw)
        b = step_records(eng, out.past_key_values, rows, T)
    torch.cuda.synchronize()
    assert [r["op"] for r in a][-2:] == ["argmax", "spec_finish"] and len(a) > 4       # a purely greedy call keeps mg_argmax_f32
    assert [r["op"] for r in b] == [r["op"] for r in a][:-2] + ["sample_chunk", "spec_finish"]       # nothing else is added
    assert a[:-2] == b[:-2] and a[-1] == b[-1], "another launch than the selection changed"
    sel = b[-2]
    assert sel["T"] == T and sel["logits"] == a[-2]["logits"] and sel["out"] == a[-2]["out"], (sel, a[-2])
    assert sel["params"].startswith("st.sample_rows") and sel["count"].startswith("st.count") and sel["n_draft"].startswith("st.n_draft")


def test_another_calls_settings_replay_the_same_graph_and_a_greedy_call_keeps_its_own(model):  # noqa: F811
    B, T, n = 2, 4, STEPS - 1           # (a token limit no other test of this module uses: the limit is part of a graph's key)
    eng = model.lm.engine
    emb, lens, _ = prompts_of(model, B, T)
    free = eng.V - 1
    kw = dict(eos_token=[free], prompt_lookup_num_tokens=T - 1, steps=n)
    g0 = run(model, emb, lens, temperature=0.0, **kw)
    caches = [c for c in eng._cache_pool.values() if T in c.spec and any(k[1] == n for k in c.spec[T].graphs)]
    assert len(caches) == 1
    st = caches[0].spec[T]
    mine = lambda: {k: g for k, g in st.graphs.items() if k[1] == n}  # noqa: E731
    greedy_graphs = mine()
    assert len(greedy_graphs) == 1
    run(model, emb, lens, temperature=0.8, top_k=40, seed=5, **kw)
    held = mine()
    assert len(held) == 2 and all(held[k] is g for k, g in greedy_graphs.items())       # the sampled step is a graph of its own
    run(model, emb, lens, temperature=[1.1, 0.0], top_k=[5, 0], seed=[8, 9], **kw)            # other settings, a greedy row among them
    assert mine().keys() == held.keys() and all(st.graphs[k] is g for k, g in held.items())
    assert torch.equal(run(model, emb, lens, temperature=0.0, **kw), g0)
    assert mine().keys() == held.keys() and all(st.graphs[k] is g for k, g in held.items())


# ------------------------------------------------------------------------------------------------------- the quantised / unpacked step
def test_generate_w8a16_is_the_plain_sampled_call(dev, monkeypatch):
    from test_beam_search_gpu import _model
    m = _model(dev, monkeypatch, w8=True, n_head=4, mlp_factor=1)
    assert m.lm.engine.decode_w8
    sampled_cases(m, 2, 4, "reference")


def test_generate_unpacked_is_the_plain_sampled_call(dev, monkeypatch):
    from test_beam_search_gpu import _model
    monkeypatch.setenv("MAGMA_DECODE_PACK", "0")
    m = _model(dev)
    assert not m.lm.engine.decode_pack
    sampled_cases(m, 2, 4, "transformers")
