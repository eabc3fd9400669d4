"""Continuing from a KV cache on the reduced model (DESIGN.md "Continuing from a cache"):

  * LMEngine.extend: prefill(A) + extend(B) gives the logits and the cache of prefill(A || B);
  * generate(..., return_past_key_values=True) / generate(new, past_key_values=past): two and three greedy turns on a ragged batch
    with a row that stops at eos early and rows that never do equal a fresh generate over the concatenated conversation;
  * the returned cache is the caller's (another call of the same shape does not touch it), grows past its first Smax,
    KVCache.expand shares one cached prompt between several questions, sampled mode with top_k = 1 is greedy;
  * the error cases."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.fixture(scope="module")
def oracle(dev):
    """(reduced model, oracle config, oracle parameters): the model carries the oracle's seeded weights (test_model_gpu.py)."""
    from magma_amd.testing import build_reduced_magma
    from oracle.model import OracleConfig, init_params
    cfg = OracleConfig.tiny(mlp_adapter_hidden=128, attn_adapter_hidden=0)
    params = init_params(cfg, seed=11)
    for k in params:
        if ".adapter." in k:
            params[k] = params[k] * 20
    m = build_reduced_magma(dev)
    _, unexpected = m.load_checkpoint_state(params)
    assert not unexpected, unexpected
    m.eval()
    return m, cfg, {k: v for k, v in params.items() if k.startswith("lm.")}


@pytest.fixture(scope="module")
def model(oracle):
    return oracle[0]


ORACLE_MARGIN = 0.05      # greedy ids must equal the oracle's where its top-1 / top-2 gap exceeds this x std(logits)


def oracle_agree(oracle, conv, got, steps, eos, what):
    """The fp32 oracle's free-running greedy decode of one row's whole conversation, alone: its ids equal the engine's up to the
    first decision whose margin is within bf16 noise (the ids after it depend on that choice) or the engine's first eos."""
    from oracle.model import generate_greedy
    _, cfg, params = oracle
    toks, logits = generate_greedy(params, cfg, conv.float().cpu()[None], steps, stop_on_eos=False)
    ref = toks[0, conv.shape[0]:].tolist()
    n_checked = 0
    for i, x in enumerate(got):
        top2 = torch.topk(logits[i][0], 2).values
        if float(top2[0] - top2[1]) <= ORACLE_MARGIN * float(logits[i][0].std()):
            break
        assert x == ref[i], f"{what}: token {i}: engine {x} != oracle {ref[i]} (oracle ids {ref})"
        n_checked += 1
        if x == eos:
            break
    return n_checked


def embeds(model, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    d = model.lm.config.hidden_size
    return [(torch.randn(n, d, generator=g) * 0.5).to(BF16).to(model.device) for n in lengths]


def gen(model, inputs, steps, eos, **kw):
    from magma_amd.sampling import generate
    return generate(model, inputs, max_steps=steps, temperature=0.0, eos_token=eos, decode=False, **kw)


def new_tokens(out, lengths, eos, steps=None):
    """Row b's generated ids (up to and including its first eos) of generate()'s (B, s + n) output."""
    rows = []
    for b, n in enumerate(lengths):
        t = out[b, n: None if steps is None else n + steps].tolist()
        rows.append(t[: t.index(eos) + 1] if eos in t else t)
    return rows


def agree(model, convs, got, ref, what):
    """Continued and fresh ids of every row are equal, or first differ where the fresh run's two candidates are tied to within
    bf16 rounding (continuation and fresh prefill add in different orders): 2 % of the logits' spread."""
    wte = model.lm.engine.wte
    for b, (conv, g, r) in enumerate(zip(convs, got, ref)):
        for i, (x, y) in enumerate(zip(g, r)):
            if x != y:
                ctx = torch.cat([conv, wte[torch.tensor(r[:i], dtype=torch.long, device=conv.device)]], 0)[None]
                lg = model.lm(inputs_embeds=ctx).logits[0, -1].float()
                gap = abs(float(lg[x] - lg[y]))
                assert gap <= 0.02 * float(lg.std()), f"{what}, row {b}, token {i}: {x} != {y}, fresh margin {gap:.4f}"
                break
        else:
            assert len(g) == len(r), f"{what}, row {b}: {g} != {r}"


def kept(tokens, eos):
    return tokens[: tokens.index(eos)] if eos in tokens else tokens


def test_extend_matches_prefill_of_the_concatenation(model):
    eng = model.lm.engine
    dev, d = model.device, model.lm.config.hidden_size
    B, SA, SB = 3, 40, 23
    g = torch.Generator().manual_seed(5)
    a = (torch.randn(B, SA, d, generator=g) * 0.5).to(BF16).to(dev)
    bb = (torch.randn(B, SB, d, generator=g) * 0.5).to(BF16).to(dev)
    ref = model.lm(inputs_embeds=torch.cat([a, bb], 1))                       # cacheless forward: (B, SA+SB, V) logits
    ref_c = model.lm(inputs_embeds=torch.cat([a, bb], 1), use_cache=True)
    o = model.lm(inputs_embeds=a, use_cache=True)
    cache = o.past_key_values
    e = model.lm(inputs_embeds=bb, past_key_values=cache, use_cache=True)
    assert e.past_key_values is cache and cache.pos == SA + SB and cache.d_pos.tolist() == [SA + SB]
    assert rel(e.logits[:, -1], ref_c.logits[:, -1]) < 2e-2
    assert rel(e.full_logits, ref.logits[:, SA:]) < 2e-2
    n = SA + SB
    assert rel(cache.k[:, :, :, :n], ref_c.past_key_values.k[:, :, :, :n]) < 1e-2
    assert rel(cache.v[:, :, :, :n], ref_c.past_key_values.v[:, :, :, :n]) < 1e-2
    # ragged chunk: row b appends lengths[b] rows at its own position
    lens_a, lens_b = [40, 17, 29], [23, 5, 11]
    o = model.lm(inputs_embeds=a, use_cache=True, lengths=lens_a)
    cache = o.past_key_values
    e = model.lm(inputs_embeds=bb, past_key_values=cache, use_cache=True, lengths=lens_b)
    assert cache.d_pos.tolist() == [x + y for x, y in zip(lens_a, lens_b)]
    for r in range(B):
        cat = torch.cat([a[r:r + 1, : lens_a[r]], bb[r:r + 1, : lens_b[r]]], 1)
        f = model.lm(inputs_embeds=cat)
        assert rel(e.logits[r, -1], f.logits[0, -1]) < 2e-2, f"row {r}"
        assert rel(e.full_logits[r, : lens_b[r]], f.logits[0, lens_a[r]:]) < 2e-2, f"row {r}"
        m = lens_a[r] + lens_b[r]
        fc = model.lm(inputs_embeds=cat, use_cache=True).past_key_values
        assert rel(cache.k[:, r, :, :m], fc.k[:, 0, :, :m]) < 1e-2 and rel(cache.v[:, r, :, :m], fc.v[:, 0, :, :m]) < 1e-2


def _turns(model, prompts, questions, steps, eos, oracle=None):
    """Multi-turn run: returns per turn the generated ids of every row, plus the same ids from fresh generate calls over the
    concatenated conversations; with ``oracle``, every row of every turn is also checked against the fp32 oracle run on that
    row's conversation alone (returns the number of ids so checked as well)."""
    wte = model.lm.engine.wte
    n_oracle = 0
    got, fresh = [], []
    conv = [p.clone() for p in prompts]
    out, past = gen(model, prompts, steps, eos, return_past_key_values=True)
    toks = new_tokens(out, [p.shape[0] for p in prompts], eos, steps)
    got.append(toks)
    if oracle is not None:
        n_oracle += sum(oracle_agree(oracle, c, t, steps, eos, f"turn 1, row {b}") for b, (c, t) in enumerate(zip(conv, toks)))
    for turn, q in enumerate(questions, start=2):
        conv = [torch.cat([c, wte[torch.tensor(kept(t, eos), dtype=torch.long, device=c.device)], qq], 0)
                for c, t, qq in zip(conv, toks, q)]
        out, past = gen(model, q, steps, eos, past_key_values=past, return_past_key_values=True)
        toks = new_tokens(out, [x.shape[0] for x in q], eos, steps)
        got.append(toks)
        fo = gen(model, conv, steps, eos)
        fresh.append(new_tokens(fo, [c.shape[0] for c in conv], eos, steps))
        agree(model, conv, toks, fresh[-1], f"turn {turn}")
        if oracle is not None:
            n_oracle += sum(oracle_agree(oracle, c, t, steps, eos, f"turn {turn}, row {b}") for b, (c, t) in enumerate(zip(conv, toks)))
    return got, fresh, past, n_oracle


def _pick_eos(model, prompts, steps):
    """An eos id that row 0 emits early (its 3rd token) and no other row emits within `steps` tokens."""
    out = gen(model, prompts, steps, -7)
    rows = new_tokens(out, [p.shape[0] for p in prompts], -7, steps)
    assert len({tuple(r) for r in rows}) == len(rows), f"the rows' outputs are not distinct: {rows}"
    for cand in [rows[0][2], rows[0][1], rows[0][3]]:
        if all(cand not in r for r in rows[1:]) and rows[0].index(cand) >= 1:
            return cand
    raise AssertionError(f"no token of row 0's steps 1-3 is absent from the other rows: {rows}")


def test_two_and_three_turns_equal_fresh_generate_and_the_oracle(model, oracle):
    prompts = embeds(model, [30, 12, 21], seed=11)
    steps = 9
    eos = _pick_eos(model, prompts, steps)
    questions = [embeds(model, [5, 9, 1], seed=12), embeds(model, [7, 3, 4], seed=13)]
    got, fresh, past, n_oracle = _turns(model, prompts, questions, steps, eos, oracle)
    assert eos in got[0][0] and all(eos not in r for r in got[0][1:]), "turn 1 must stop row 0 at eos and no other row"
    assert past.ragged and past.B == 3
    # 3 turns x 3 rows: a good share of the ids the rows generated were checked against the oracle
    assert n_oracle >= 0.3 * sum(len(t) for turn in got for t in turn), n_oracle


def test_the_returned_cache_is_the_callers(model):
    prompts = embeds(model, [20, 20], seed=21)
    q = embeds(model, [6, 6], seed=22)
    out1, past = gen(model, prompts, 6, -7, return_past_key_values=True)
    k_before, v_before = past.k.clone(), past.v.clone()
    gen(model, embeds(model, [20, 20], seed=23), 6, -7)                     # same shape, other prompts
    # bit patterns: the slots past the conversation hold whatever the allocation held (NaN patterns included)
    assert torch.equal(past.k.view(torch.int16), k_before.view(torch.int16))
    assert torch.equal(past.v.view(torch.int16), v_before.view(torch.int16))
    a = gen(model, q, 6, -7, past_key_values=past)
    _, past2 = gen(model, prompts, 6, -7, return_past_key_values=True)
    gen(model, embeds(model, [20, 20], seed=24), 6, -7)
    b = gen(model, q, 6, -7, past_key_values=past2)
    assert torch.equal(a, b)


def test_growth_past_the_first_smax(model):
    prompts = embeds(model, [40, 33], seed=31)
    out, past = gen(model, prompts, 4, -7, return_past_key_values=True)
    smax0 = past.Smax
    q = embeds(model, [smax0 - 40, 20], seed=32)                             # row 0 runs past the first cache
    a = gen(model, q, 4, -7, past_key_values=past, return_past_key_values=True)[0]
    assert past.Smax > smax0
    t0 = new_tokens(out, [40, 33], -7)
    wte = model.lm.engine.wte
    conv = [torch.cat([p, wte[torch.tensor(t, dtype=torch.long, device=p.device)], x], 0) for p, t, x in zip(prompts, t0, q)]
    f = gen(model, conv, 4, -7)
    agree(model, conv, new_tokens(a, [x.shape[0] for x in q], -7, 4), new_tokens(f, [c.shape[0] for c in conv], -7, 4), "growth")


def test_shared_prefix_expand(model):
    prefix = embeds(model, [37], seed=41)[0]
    qs = embeds(model, [3, 8, 5, 1, 12, 6, 9, 4], seed=42)
    cache = model.cache_prompt(prefix[None])
    big = cache.expand(8)
    assert big.B == 8 and big.rows_pos().tolist() == [37] * 8
    a = gen(model, qs, 7, -7, past_key_values=big)
    conv = [torch.cat([prefix, q], 0) for q in qs]
    f = gen(model, conv, 7, -7)
    agree(model, conv, new_tokens(a, [q.shape[0] for q in qs], -7, 7), new_tokens(f, [37 + q.shape[0] for q in qs], -7, 7), "shared prefix")
    # the prompt-only cache itself is untouched and can be expanded again
    assert cache.rows_pos().tolist() == [37] and cache.expand(2).B == 2


def test_sampled_top1_equals_greedy(model):
    from magma_amd.sampling import generate
    prompts = embeds(model, [25, 14], seed=51)
    q = embeds(model, [4, 10], seed=52)
    _, p1 = gen(model, prompts, 5, -7, return_past_key_values=True)
    g = gen(model, q, 5, -7, past_key_values=p1)
    _, p2 = generate(model, prompts, max_steps=5, temperature=1.0, top_k=1, top_p=0.0, eos_token=-7, decode=False, seed=9,
                     return_past_key_values=True)
    s = generate(model, q, max_steps=5, temperature=1.0, top_k=1, top_p=0.0, eos_token=-7, decode=False, seed=9, past_key_values=p2)
    assert torch.equal(g, s)


def test_error_cases(model):
    prompts = embeds(model, [10, 10], seed=61)
    _, past = gen(model, prompts, 3, -7, return_past_key_values=True)
    with pytest.raises(NotImplementedError):
        model.generate(embeds(model, [4, 4], seed=62), num_beams=2, past_key_values=past, decode=False)
    with pytest.raises(NotImplementedError):
        model.generate(prompts, num_beams=2, return_past_key_values=True, decode=False)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        n = model.lm.config.max_position_embeddings
        gen(model, embeds(model, [n, 4], seed=63), 2, -7, past_key_values=past)
    with pytest.raises(ValueError):                                          # a row with no new input
        e = torch.zeros(2, 4, model.lm.config.hidden_size, dtype=BF16, device=model.device)
        gen(model, e, 2, -7, past_key_values=past, lengths=[4, 0])
    with pytest.raises(ValueError):                                          # rows of the cache vs rows of the input
        gen(model, embeds(model, [4, 4, 4], seed=64), 2, -7, past_key_values=past)
