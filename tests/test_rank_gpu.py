"""Ranking choices on the engine (DESIGN.md "Ranking choices"): Magma.rank -- one prefill, one tree forward per group of choices --
against Magma.score on every candidate (one cache-less forward each), term by term under the project's cross-path rule
(SURVEY 8(c)): d <= 2 e_bf16 + 1e-2, e_bf16 the difference between the CPU oracle in eager bf16 and in fp32 on the same tokens.
Then the index against score's sums, a case choose() gets wrong, grouping, the cache left as it was, MAGMA_v2 blocks, an fp8
prefill switch, and the full-width vocabulary."""
import pytest
import torch

from test_beam_search_gpu import _model

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LENS = (5, 9, 2)


def _oracle_model(dev, attn=False):
    """(reduced model carrying the CPU oracle's seeded weights, oracle config, the oracle's LM parameters), as the fixture of
    tests/test_logprobs_gpu.py; ``attn``: MAGMA_v2 blocks (an attention adapter as well)."""
    from magma_amd.testing import build_reduced_magma
    from oracle.model import OracleConfig, init_params
    cfg = OracleConfig.tiny(mlp_adapter_hidden=128, attn_adapter_hidden=64 if attn else 0)
    params = init_params(cfg, seed=11)
    for k in params:
        if ".adapter." in k:
            params[k] = params[k] * 20
    m = build_reduced_magma(dev, attn_factor=8 if attn else None)
    _, unexpected = m.load_checkpoint_state(params)
    assert not unexpected, unexpected
    m.eval()
    return m, cfg, {k: v for k, v in params.items() if k.startswith("lm.")}


@pytest.fixture(scope="module")
def oracle(dev):
    return _oracle_model(dev)


def _prompts(model, lens=LENS, seed=31):
    g = torch.Generator().manual_seed(seed)
    d = model.lm.config.hidden_size
    return [(torch.randn(n, d, generator=g) * 0.5).to(BF16).to(model.device) for n in lens]


def _choices(V, eos, seed, count=7):
    """1 to 5 ids with shared prefixes, one choice a prefix of another, one listed twice."""
    g = torch.Generator().manual_seed(seed)
    t = [v for v in torch.randperm(V, generator=g).tolist() if v != eos][:24]
    seqs = [[t[0]], [t[1], t[2]], [t[1], t[2], t[3]], [t[1], t[4], t[5], t[6]], [t[7], t[8], t[9], t[10], t[11]], [t[7], t[8], t[12]],
            [t[13]], [t[14], t[15]], [t[16], t[17], t[18]]][:count]
    return seqs + [seqs[1]]


def _score_terms(model, prompt, seqs, eos):
    """Magma.score on every candidate of one row: [C] lists of its terms (the eos term last)."""
    tg = [list(q) + [eos] for q in seqs]
    sc = model.score([prompt] * len(seqs), tg)
    return [sc.logprobs[c, : len(tg[c])].double() for c in range(len(seqs))]


def _e_bf16(cfg, params, prompts, rows, eos):
    """max |lp| difference between the CPU oracle in eager bf16 and in fp32, teacher-forced on every candidate (+ eos)."""
    from oracle.model import lm_forward
    p16 = {k: v.to(BF16) for k, v in params.items()}
    wte = params["lm.transformer.wte.weight"]
    e = 0.0
    for p, seqs in zip(prompts, rows):
        for q in {tuple(q) for q in seqs}:
            toks = torch.tensor(list(q) + [eos])
            seq = torch.cat([p.float().cpu(), wte[toks[:-1]].to(BF16).float()], 0)[None]
            lp = []
            for prm, x in ((params, seq), (p16, seq.to(BF16))):
                lg = lm_forward(prm, cfg, inputs_embeds=x)["logits"][0, p.shape[0] - 1:].double()
                lp.append(torch.log_softmax(lg, -1).gather(1, toks[:, None])[:, 0])
            e = max(e, float((lp[0] - lp[1]).abs().max()))
    return e


def _check_against_score(model, cfg, params, prompts, rows, what, choices=None):
    """Every term of rank's sums within 2 e_bf16 + 1e-2 of score's; the index is the arg-max of score's sums, which are apart
    by more than 2 * count * that bound.  Returns (ranking, terms, bound)."""
    eos = model.eos_token
    got, terms = model.rank(prompts, rows if choices is None else choices, return_terms=True)
    e = _e_bf16(cfg, params, prompts, rows, eos)
    bound = 2 * e + 1e-2
    d = 0.0
    for b, seqs in enumerate(rows):
        ref = _score_terms(model, prompts[b], seqs, eos)
        sums = torch.stack([t.sum() for t in ref])
        for c, t in enumerate(ref):
            assert int(got.count[b, c]) == len(t)
            d = max(d, float((terms[b, c, : len(t)].double() - t).abs().max()))
            assert not terms[b, c, len(t):].any()
            assert abs(float(got.logprobs[b, c]) - float(terms[b, c].double().sum())) <= 1e-5
        top = torch.sort(sums, descending=True)[0]
        gap, need = float(top[0] - top[1]), 2 * int(got.count[b].max()) * bound
        print(f"{what}: row {b}: best two sums of score {gap:.3f} apart, needed {need:.3f}")
        assert gap > need, (what, b, gap, need)
        assert int(got.index[b]) == int(torch.argmax(sums)), (what, b)
    print(f"{what}: cross-path d = {d:.4e}, e_bf16 = {e:.4e}, bound {bound:.4e}")
    assert d <= bound, (what, d, e)
    return got, terms, bound


# The seeds of the choices were picked on the CPU with the oracle in fp32, over seeds 0 .. 13: with these the best two sums of every
# row -- under the MAGMA_v1 and under the MAGMA_v2 parameters, for the shared trie (seed 0 on all rows) and for one trie per row
# -- are at least 0.79 apart, where 2 * count * (2 e_bf16 + 1e-2) comes to about 0.4 (e_bf16 about 0.01, count <= 6); the choice
# that is listed twice is never the best one.
SEEDS = (0, 3, 5)


def test_rank_against_score_per_token(oracle):
    """B = 3 ragged prompts; one shared trie, then one trie per row."""
    model, cfg, params = oracle
    prompts = _prompts(model)
    V, eos = model.lm.engine.V, model.eos_token
    shared = _choices(V, eos, SEEDS[0], count=9)
    got, _, _ = _check_against_score(model, cfg, params, prompts, [shared] * 3, "shared trie", choices=shared)
    assert got.logprobs.shape == (3, 10) and torch.equal(got.logprobs[:, 1], got.logprobs[:, 9])       # the duplicate, twice
    assert torch.equal(got.scores, got.logprobs)                                                       # length_penalty = 0
    rows = [_choices(V, eos, SEEDS[b], count=5 + 2 * b) for b in range(3)]
    got, _, _ = _check_against_score(model, cfg, params, prompts, rows, "one trie per row")
    assert got.logprobs.shape == (3, 10) and bool(torch.isinf(got.logprobs[0, 6:]).all()) and not got.count[0, 6:].any()
    # length_penalty and eos only change the bookkeeping
    pen = model.rank(prompts, rows, length_penalty=1.0)
    assert torch.equal(pen.logprobs, got.logprobs)
    live = got.count > 0
    assert torch.allclose(pen.scores[live], (got.logprobs / got.count.clamp(min=1))[live], rtol=1e-6, atol=0)
    no_eos, t0 = model.rank(prompts, rows, eos=False, return_terms=True)
    _, t1 = model.rank(prompts, rows, return_terms=True)
    assert torch.equal(no_eos.count[live], got.count[live] - 1)
    for b, seqs in enumerate(rows):
        for c, q in enumerate(seqs):
            assert torch.equal(t0[b, c, : len(q)], t1[b, c, : len(q)]) and float(t0[b, c, len(q)]) == 0.0
    # the padded-tensor form of the prompt
    from magma_amd.sampling import pad_ragged
    emb, lens = pad_ragged(prompts)
    again = model.rank(emb, rows, lengths=lens)
    assert torch.equal(again.logprobs, got.logprobs) and torch.equal(again.index, got.index)
    assert torch.equal(model.rank((emb, lens), rows).logprobs, got.logprobs)


def test_rank_is_not_choose(oracle):
    """The greedy path wins the first token and loses overall: choice A = one token, the fifth most probable after the prompt;
    choice B starts with THE most probable token and goes on with two arbitrary ones.  choose() walks into B, rank() -- and
    score's sums -- prefer A."""
    model, cfg, params = oracle
    prompts = _prompts(model, seed=33)
    eng = model.lm.engine
    from magma_amd.sampling import pad_ragged
    emb, lens = pad_ragged(prompts)
    logits, _, _ = eng.prefill(emb, lengths=lens)
    top = torch.topk(logits.float(), 6, dim=-1)[1].cpu()
    eos = model.eos_token
    rows = []
    for b in range(3):
        first = [int(t) for t in top[b] if int(t) != eos]
        rows.append([[first[0], 17 + b, 400 + b], [first[4]], [first[0], 17 + b, 401 + b]])
    got, _, _ = _check_against_score(model, cfg, params, prompts, rows, "rank against choose")
    index, _ = model.choose(prompts, rows)
    assert got.index.tolist() == [1, 1, 1]
    assert all(int(i) in (0, 2) for i in index), index


def test_grouping_keeps_the_bits(oracle):
    """With the nodes per forward capped the trie goes through in groups of whole choices, each against the same prompt cache: the
    first group's nodes sit in the rows they have in the whole trie, so its choices keep their bits; the others keep their
    values within the cross-path bound, and the index stays."""
    from magma_amd.sampling import TokenTrie, rank_groups
    model, cfg, params = oracle
    prompts = _prompts(model)
    V, eos = model.lm.engine.V, model.eos_token
    rows = [_choices(V, eos, SEEDS[b], count=9) for b in range(3)]
    whole, tw = model.rank(prompts, rows, return_terms=True)
    for cap in (6, 9):
        part, tp = model.rank(prompts, rows, max_nodes=cap, return_terms=True)
        assert torch.equal(part.index, whole.index) and torch.equal(part.count, whole.count)
        moved = 0
        for b, seqs in enumerate(rows):
            groups = rank_groups(TokenTrie(seqs), cap)
            assert len(groups) > 1
            for c in groups[0]:
                assert torch.equal(tp[b, c], tw[b, c]) and float(part.logprobs[b, c]) == float(whole.logprobs[b, c]), (cap, b, c)
            moved += sum(len(g) for g in groups[1:])
        assert moved > 0
        e = _e_bf16(cfg, params, prompts, rows, eos)
        assert float((tp - tw).abs().max()) <= 2 * e + 1e-2
    with pytest.raises(ValueError):
        model.rank(prompts, rows, max_nodes=4)                 # a choice of five tokens


def test_tree_forward_leaves_the_cache_intact(oracle):
    from magma_amd.sampling import TokenTrie, pad_trie_rows
    model, _, _ = oracle
    prompts = _prompts(model, seed=35)
    question = _prompts(model, (3, 1, 4), seed=36)
    eng = model.lm.engine
    used, fresh = model.cache_prompt(prompts), model.cache_prompt(prompts)
    k0, v0, pos0 = used.k.clone(), used.v.clone(), used.rows_pos().clone()
    rows = TokenTrie(_choices(eng.V, model.eos_token, 5, count=9)).rows()
    x = eng.tree_forward(used, pad_trie_rows([rows] * 3))
    assert x.shape == (3 * rows.token.numel(), eng.d) and bool(torch.isfinite(x.float()).all())
    assert torch.equal(used.rows_pos(), pos0) and torch.equal(used.d_pos.cpu(), fresh.d_pos.cpu()) and used.pending is None
    for b, p in enumerate(pos0.tolist()):
        assert torch.equal(used.k[:, b, :, :p], k0[:, b, :, :p]) and torch.equal(used.v[:, b, :, :p], v0[:, b, :, :p])
        assert not torch.equal(used.k[:, b, :, p:p + 4], k0[:, b, :, p:p + 4])            # the scratch slots were used
    kw = dict(max_steps=6, temperature=0.0, decode=False, stop_on_eos=False)
    a = model.generate(question, past_key_values=used, **kw)
    b_ = model.generate(question, past_key_values=fresh, **kw)
    assert torch.equal(a, b_)
    with pytest.raises(ValueError):
        eng.tree_forward(fresh, pad_trie_rows([rows] * 2))
    with pytest.raises(TypeError):
        eng.tree_forward(None, pad_trie_rows([rows] * 3))


@pytest.mark.parametrize("kind", ["v2", "fp8"])
def test_switches_and_variants(dev, monkeypatch, kind):
    """MAGMA_v2 blocks (an attention adapter beside the MLP adapter), and the fp8 prefill GEMMs (MAGMA_FP8=all; the attention core
    stays bf16 on both sides, MAGMA_FP8_ATTN=0: a cached chunk has no fp8 attention): rank against score under the same switch."""
    if kind == "fp8":
        monkeypatch.setenv("MAGMA_FP8", "all")
        monkeypatch.setenv("MAGMA_FP8_ATTN", "0")
    model, cfg, params = _oracle_model(dev, attn=kind == "v2")
    eng = model.lm.engine
    assert (eng.fp8_mode == "all") == (kind == "fp8") and (eng.layers[0].attn_adapter is not None) == (kind == "v2")
    prompts = _prompts(model)
    rows = [_choices(eng.V, model.eos_token, SEEDS[b], count=5 + 2 * b) for b in range(3)]
    _check_against_score(model, cfg, params, prompts, rows, kind)


def test_full_width_vocabulary(dev):
    """d = 4096, V = 50 258, one block, B = 2, a trie of a few hundred choices: rank against score, term by term.  No CPU oracle
    of this width is at hand, so the bound is the rule's constant alone, 1e-2 (e_bf16 >= 0: never wider than the rule)."""
    model = _model(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=128)
    eos = model.eos_token
    g = torch.Generator().manual_seed(90)
    emb = torch.randn(2, 5, model.lm.config.hidden_size, generator=g).to(BF16).to(model.device)
    t = [v for v in torch.randperm(50258, generator=g).tolist() if v != eos]
    seqs = [t[3 * i: 3 * i + 1 + i % 3] for i in range(300)]
    seqs += [[q[0], t[1000 + i]] for i, q in enumerate(seqs[:40])]                  # shared first tokens
    got, terms = model.rank(emb, seqs, return_terms=True)
    assert got.logprobs.shape == (2, 340) and bool(torch.isfinite(got.logprobs).all())
    pick = list(range(0, 340, 17)) + [300, 339]
    d = 0.0
    for b in range(2):
        ref = _score_terms(model, emb[b], [seqs[c] for c in pick], eos)
        for c, r in zip(pick, ref):
            d = max(d, float((terms[b, c, : len(r)].double() - r).abs().max()))
    print(f"full width: cross-path d = {d:.4e}, bound 1e-2")
    assert d <= 1e-2, d
