"""Speculative greedy decoding on the engine (DESIGN.md "Speculative decoding"), on the reduced model of
tests/test_continue_generate_gpu.py.

The feature is exact by construction, so every comparison is an equality:
  * one speculative step over (B, T) gives the logits bits of one plain step over a cache of B * T rows, each holding the prefilled
    prompt and teacher-forced to its own position with the same ids -- the chunk attention and the M = B * T GEMVs are the plain step's;
  * generate(prompt_lookup_num_tokens = T - 1) is token for token the per-row greedy call, whatever the lookup ids are -- under the
    asserted precondition that the plain greedy ids of the prompts agree between the B-row call and the B * T-row call on the prompts
    repeated (the step's GEMVs run over B * T rows; the claim is about the speculation, not about GEMV shapes);
  * the launches of the speculative step are the greedy step's with the attention launches and the bookkeeping launch replaced, and
    a plain call on the same pooled cache keeps its captured graphs."""
import math

import pytest
import torch

from test_continue_generate_gpu import embeds, model, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
STEPS = 24
LENS = [40, 3, 65]
SHAPES = [(1, 8), (2, 4), (3, 5), (2, 8)]


def padded(m, prompts):
    emb = torch.zeros(len(prompts), max(p.shape[0] for p in prompts), prompts[0].shape[1], dtype=BF16, device=m.device)
    for r, p in enumerate(prompts):
        emb[r, : p.shape[0]] = p
    return emb, [p.shape[0] for p in prompts]


def tokens(out, lens, steps=STEPS):
    return [out[b, n: n + steps].tolist() for b, n in enumerate(lens)]


# ------------------------------------------------------------------------------------------------------------------ the engine
@pytest.mark.parametrize("pack", ["default", "0", "two_launches"])
@pytest.mark.parametrize("B,T", SHAPES[:3])
def test_one_speculative_step_has_the_bits_of_the_plain_step_over_BT_rows(dev, monkeypatch, B, T, pack):
    from test_beam_search_gpu import _model
    if pack == "0":
        monkeypatch.setenv("MAGMA_DECODE_PACK", "0")
    if pack == "two_launches":          # the chunk attention and the GEMV as two launches: the same bits are claimed for it
        monkeypatch.setenv("MAGMA_SPEC_COLAUNCH", "0")
    m = _model(dev)
    eng = m.lm.engine
    assert eng.decode_pack == (pack != "0")
    emb, lens = padded(m, embeds(m, LENS[:B], seed=31))
    ids = torch.randint(0, eng.V, (B, T), generator=torch.Generator().manual_seed(B * 10 + T)).to(dev)
    with torch.no_grad():
        # the plain statement: row b * T + t holds prompt b and ids[b, :t], then takes ids[b, t] in one step over all B * T rows
        # (every row is the SAME prefill, copied T times: a prefill of B * T rows picks other GEMM splits than one of B rows, which
        # is not what is compared here -- the end-to-end test states that precondition for whole calls)
        lens_r = torch.tensor(lens).repeat_interleave(T)
        _, cache, _ = eng.prefill(emb, cache_hint=T + 8, lengths=torch.tensor(lens))
        wide = cache.expand(T)
        t_of = torch.arange(T).repeat(B)
        for j in range(T - 1):          # round j forces ids[b, j]; a row that is already at its position is put back there
            eng.decode(ids[:, j].repeat_interleave(T).view(B * T, 1), wide, use_graph=False, select=False)
            wide.set_rows(lens_r + torch.minimum(t_of, torch.tensor(j + 1)))
        want, _ = eng.decode(ids.reshape(B * T, 1), wide, use_graph=False, select=False)
        want = want.clone()
        got = eng.decode_chunk(ids, cache)
        assert cache.spec[T].colaunch == (pack != "two_launches")
        torch.cuda.synchronize()
        assert got.shape == want.shape == (B * T, eng.V) and not bool(got.isnan().any())
        assert torch.equal(got, want), f"rows {(got != want).any(1).nonzero().flatten().tolist()} differ"
        for b in range(B):              # and the cache holds what the last row of the sequence's group holds
            n = lens[b] + T
            assert torch.equal(cache.k[:, b, :, :n], wide.k[:, b * T + T - 1, :, :n])
            assert torch.equal(cache.v[:, b, :, :n], wide.v[:, b * T + T - 1, :, :n])
        assert cache.d_pos.tolist() == lens                                     # teacher-forced: nothing advanced


# ------------------------------------------------------------------------------------------------------------------ end to end
def greedy(m, emb, lens, steps=STEPS, **kw):
    from magma_amd.sampling import generate
    return generate(m, emb, lengths=lens, max_steps=steps, temperature=0.0, decode=False, **kw)


def free_ids(m, rows, n):
    """n token ids no row of ``rows`` holds (and not the image token): eos ids that never fire, replacement tokens."""
    used = {t for r in rows for t in r} | {m.image_token}
    return [t for t in range(m.lm.engine.V) if t not in used][:n]


def speculative_cases(m, B, T):
    from magma_amd.sampling import generate
    emb, lens = padded(m, embeds(m, LENS[:B], seed=22))
    long = tokens(greedy(m, emb, lens, STEPS + 8, eos_token=-7), lens, STEPS + 8)          # the lookup text: the greedy output, and 8 more
    g = [r[:STEPS] for r in long]
    wide = tokens(greedy(m, emb.repeat_interleave(T, 0), [n for n in lens for _ in range(T)], eos_token=-7), [n for n in lens for _ in range(T)])
    assert wide == [r for r in g for _ in range(T)], "pick other prompts: these decode differently at B and at B * T rows already"
    free = free_ids(m, long, 4)
    eos_mid = g[0][9]                    # row 0 finishes mid-run, inside an accepted run; the other rows go on
    third = [[free[3] if i % 3 == 2 else t for i, t in enumerate(r)] for r in long]
    for eos in ([free[0]], [eos_mid], [free[0], eos_mid, free[1]]):
        kw = dict(eos_token=eos, stop_per_row=True, return_finish=True)
        want, fin = greedy(m, emb, lens, **kw)
        for name, lookup in (("itself", long), ("third", third), ("none", None)):
            got, fin2, sp = generate(m, emb, lengths=lens, max_steps=STEPS, temperature=0.0, decode=False, prompt_lookup_num_tokens=T - 1,
                                     max_matching_ngram_size=8, lookup_ids=lookup, return_speculation=True, **kw)
            what = f"B={B} T={T} eos={eos} lookup={name}"
            assert torch.equal(got, want), f"{what}: {tokens(got, lens)} != {tokens(want, lens)}"
            assert torch.equal(fin2.kept, fin.kept) and fin2.reason == fin.reason and fin2.index == fin.index, what
            assert bool((sp.accepted <= sp.drafted).all()) and bool((sp.steps >= 1).all()), what
            if eos_mid in eos:
                assert fin.reason[0] == "eos" and int(fin.kept[0]) == g[0].index(eos_mid) + 1 < STEPS, what
            if name == "itself" and eos == [free[0]]:
                # the text to look up is the answer: every draft is right (n-grams of up to 8 tokens find the answer's own place)
                assert torch.equal(sp.accepted, sp.drafted) and int(sp.drafted.min()) > 0, (what, sp)
                assert int(sp.steps.max()) <= math.ceil(STEPS / T) + 1, (what, sp)
            if name == "third" and eos == [free[0]]:
                assert int(sp.accepted.min()) > 0 and int(sp.steps.max()) < STEPS, (what, sp)


@pytest.mark.parametrize("B,T", SHAPES)
def test_generate_is_the_greedy_call_token_for_token(model, B, T):  # noqa: F811
    speculative_cases(model, B, T)


def test_generate_w8a16_is_the_greedy_call_token_for_token(dev, monkeypatch):
    from test_beam_search_gpu import _model
    m = _model(dev, monkeypatch, w8=True, n_head=4, mlp_factor=1)
    assert m.lm.engine.decode_w8
    speculative_cases(m, 2, 4)


# ---------------------------------------------------------------------------------------------------------------- the launches
def step_records(eng, cache, plan, state=None):
    """tests/launch_trace.py's records of one eager token step on ``cache``: every op with every argument, buffers by name.
    ``state``: the decode state whose fields the names ``st.*`` mean (the speculative step's lives in cache.spec[T])."""
    import launch_trace as lt
    held = cache.decode_state
    if state is not None:
        cache.decode_state = state
    try:
        recs, res = lt.record(eng, lambda: eng.decode(None, cache, use_graph=False, plan=plan), cache=cache,
                              op_names=lt.OPS + ("sample_finish_rows", "attn_decode_chunk", "spec_finish"))
    finally:
        cache.decode_state = held
    if isinstance(res, Exception):
        raise res
    return recs


@pytest.mark.parametrize("T", [4, 8])
def test_the_speculative_step_is_the_greedy_step_with_three_launches_replaced(model, T):  # noqa: F811
    """Record for record against the plain per-row greedy step over B * T rows: the same ops on the same weights and the same
    buffers of the decode state, except the attention launches (the chunk forms, over the cache's B rows), the ids the embedding
    reads (the step's own id buffer) and the bookkeeping launch."""
    from magma_amd.engine import LMEngine
    eng, B = model.lm.engine, 2
    emb, lens = padded(model, embeds(model, LENS[:B], seed=22))
    stop = dict(eos_ids=(model.eos_token,), stop_seqs=())
    plain = LMEngine.selection_plan(stop=stop, vocab=eng.V)
    spec = LMEngine.selection_plan(stop=stop, speculate=(T, 2), vocab=eng.V)
    with torch.no_grad():
        out = model.lm(inputs_embeds=emb.repeat_interleave(T, 0), use_cache=True, cache_hint=STEPS + T, eos_token=model.eos_token,
                       plan=plain, lengths=[n for n in lens for _ in range(T)])
        a = step_records(eng, out.past_key_values, plain)
        out = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=STEPS + T, eos_token=model.eos_token, plan=spec, lengths=lens,
                       seed=dict(limit=STEPS, lookup=None))
        b = step_records(eng, out.past_key_values, spec, state=out.past_key_values.spec[T])
    torch.cuda.synchronize()
    swap = {"decode_attn_gemv": "decode_attn_gemv", "attn_decode_fused": "attn_decode_chunk", "sample_finish_rows": "spec_finish"}
    assert [r["op"] for r in a][-2:] == ["argmax", "sample_finish_rows"] and any(r["op"] in swap for r in a[:-1]), a
    assert [r["op"] for r in b] == [swap.get(r["op"], r["op"]) for r in a]
    for ra, rb in zip(a, b):
        if ra["op"] == "decode_attn_gemv":
            assert rb.get("chunk") == T and rb["B"] == B and ra["B"] == B * T and "chunk" not in ra
            assert (ra["qkv"], ra["attn_out"], ra["gemv"]) == (rb["qkv"], rb["attn_out"], rb["gemv"]), (ra, rb)
        elif ra["op"] == "attn_decode_fused":
            assert rb["T"] == T and rb["B"] == B and (ra["qkv"], ra["out"]) == (rb["qkv"], rb["out"]), (ra, rb)
        elif ra["op"] == "embedding":
            assert {k: v for k, v in ra.items() if k != "ids"} == {k: v for k, v in rb.items() if k != "ids"}, (ra, rb)
        elif ra["op"] != "sample_finish_rows":
            assert ra == rb, (ra, rb)


def test_a_plain_call_on_the_same_pooled_cache_keeps_its_graphs_and_its_launches(model):  # noqa: F811
    from magma_amd.engine import LMEngine
    from magma_amd.sampling import generate
    eng = model.lm.engine
    emb, lens = padded(model, embeds(model, LENS, seed=22))
    kw = dict(eos_token=[model.eos_token], stop_per_row=True)
    plain = LMEngine.selection_plan(stop=dict(eos_ids=(model.eos_token,), stop_seqs=()), vocab=eng.V)
    first = greedy(model, emb, lens, **kw)
    first = greedy(model, emb, lens, **kw)                  # (the second call replays what the first captured)
    caches = [c for c in eng._cache_pool.values() if c.B == 3 and c.ragged and c.Smax == 128]
    assert len(caches) == 1 and caches[0].decode_state.graphs
    cache, held = caches[0], dict(caches[0].decode_state.graphs)
    with torch.no_grad():
        before = step_records(eng, cache, plain)            # the plain step's launches on this cache, every argument
    spec = generate(model, emb, lengths=lens, max_steps=STEPS, temperature=0.0, decode=False, prompt_lookup_num_tokens=4, **kw)
    assert 5 in cache.spec and cache.spec[5].graphs, "the speculative call ran on another cache than the plain call's"
    assert cache.decode_state.graphs == held and all(cache.decode_state.graphs[k] is g for k, g in held.items())
    again = greedy(model, emb, lens, **kw)
    assert torch.equal(again, first) and torch.equal(spec, first)
    assert cache.decode_state.graphs == held and all(cache.decode_state.graphs[k] is g for k, g in held.items())
    with torch.no_grad():
        after = step_records(eng, cache, plain)
    assert before and after == before                       # its old list, buffers and weights included


def test_engine_refuses_more_than_16_rows(model):  # noqa: F811
    from magma_amd.engine import LMEngine
    eng = model.lm.engine
    emb, lens = padded(model, embeds(model, LENS, seed=22))
    plan = LMEngine.selection_plan(stop=dict(eos_ids=(model.eos_token,), stop_seqs=()), speculate=(8, 2), vocab=eng.V)
    with pytest.raises(ValueError, match="at most 16"):
        model.lm(inputs_embeds=emb, use_cache=True, cache_hint=STEPS + 8, eos_token=model.eos_token, plan=plan, lengths=lens,
                 seed=dict(limit=STEPS, lookup=None))
