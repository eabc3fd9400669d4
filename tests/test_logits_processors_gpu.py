"""Logits processors on the device (DESIGN.md "Logits processors"): the kernel against the host statement
(magma_amd.sampling.process_logits, pinned to transformers by tests/test_logits_processors_cpu.py) bit for bit, its beam form
against log_softmax + the host statement, and generate(repetition_penalty=..., no_repeat_ngram_size=..., min_new_tokens=...,
suppress_tokens=...) on the reduced model -- greedy, sampled and beam search -- against the host rule driven by the engine's own
decode logits."""
import pytest
import torch

from test_beam_search_gpu import _emb, _model

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
HIST_COLS, EOS_K = 64, 3


def _bits(t):
    return t.contiguous().view(torch.int32)


def _kernel_inputs(R, V, seed):
    """fp32 rows [R, ld > V] with both signs, +0, -0 and -inf (the padding columns hold a sentinel), and histories [R, 64] from a
    small alphabet that holds the tokens of those special logits, 0 and V - 1, and one token 30 times in a row."""
    g = torch.Generator().manual_seed(seed)
    ld = V + 7
    full = torch.full((R, ld), 123.25)
    full[:, :V] = torch.randn(R, V, generator=g) * 3
    full[:, 5], full[:, 6], full[:, 7] = 0.0, -0.0, float("-inf")
    alphabet = torch.tensor([0, V - 1, 5, 6, 7, 9, 11, EOS_K, V // 2, 31])
    hist = alphabet[torch.randint(0, len(alphabet), (R, HIST_COLS), generator=g)]
    hist[:, 8:38] = 9                               # one token 30 times
    hist[:, 0], hist[:, 1], hist[:, 2:5] = 0, V - 1, torch.tensor([5, 6, 7])
    return full, hist.contiguous()


@pytest.mark.parametrize("V", [1056, 50258])
@pytest.mark.parametrize("R", [1, 5])
def test_kernel_raw_form_is_the_host_statement_bit_for_bit(dev, R, V):
    from magma_amd import ops
    from magma_amd.sampling import process_logits
    full, hist = _kernel_inputs(R, V, seed=R + V)
    hist_d = hist.to(dev)
    g = torch.Generator().manual_seed(1)
    ids17 = torch.randperm(V, generator=g)[:17].tolist()
    ids17[0], ids17[1], ids17[2] = 0, V - 1, 9
    sup_d = torch.zeros(1024, dtype=torch.int32, device=dev)
    sup_d[:17] = torch.tensor(ids17, dtype=torch.int32)
    touched = 0
    for n in (1, 2, 3):
        for step in sorted({0, 1, n - 1, n, 40, HIST_COLS}):
            state = torch.tensor([step, -1], dtype=torch.int32, device=dev)
            for penalty in (1.0, 1.3, 0.5):
                for ids in ((), tuple(ids17)):
                    rules = dict(repetition_penalty=penalty, no_repeat_ngram_size=n, min_new_tokens=45, suppress_tokens=ids)
                    want = full.clone()
                    want[:, :V] = process_logits(full[:, :V], hist, step, eos_token=EOS_K, **rules)
                    x = full.to(dev)
                    ops.logits_process(x[:, :V], state, hist_d, repetition_penalty=penalty, no_repeat_ngram_size=n,
                                       min_new_tokens=45, eos=EOS_K, suppress=sup_d, n_suppress=len(ids))
                    got = x.cpu()
                    assert torch.equal(_bits(got), _bits(want)), (n, step, penalty, len(ids), (_bits(got) != _bits(want)).nonzero()[:8])
                    touched += int(not torch.equal(_bits(want), _bits(full)))
    assert touched > 80          # of 90 combinations: the inputs exercise the rules


def test_kernel_rules_one_at_a_time_and_neutral(dev):
    """Each rule alone (the others neutral), and all neutral: the launch leaves every bit as it is."""
    from magma_amd import ops
    from magma_amd.sampling import process_logits
    R, V, step = 3, 1056, 40
    full, hist = _kernel_inputs(R, V, seed=2)
    state = torch.tensor([step, -1], dtype=torch.int32, device=dev)
    sup = torch.tensor([0, 9, V - 1], dtype=torch.int32, device=dev)
    for rules in (dict(), dict(repetition_penalty=1.7), dict(no_repeat_ngram_size=2), dict(min_new_tokens=41),
                  dict(suppress_tokens=(0, 9, V - 1))):
        want = full.clone()
        want[:, :V] = process_logits(full[:, :V], hist, step, eos_token=EOS_K, **rules)
        x = full.to(dev)
        kw = {k: v for k, v in rules.items() if k != "suppress_tokens"}
        ops.logits_process(x[:, :V], state, hist.to(dev), eos=EOS_K, suppress=sup, n_suppress=len(rules.get("suppress_tokens", ())), **kw)
        assert torch.equal(_bits(x.cpu()), _bits(want)), rules
        assert bool(rules) != torch.equal(_bits(want), _bits(full)), rules
    # neither the penalty nor the n-gram rule: no history is needed
    x = full.to(dev)
    ops.logits_process(x[:, :V], state, None, min_new_tokens=41, eos=EOS_K)
    assert bool((x[:, EOS_K] == float("-inf")).all())


@pytest.mark.parametrize("V", [1056, 50258])
def test_beam_form_against_log_softmax_and_host_statement(dev, V):
    from magma_amd import ops
    from magma_amd.sampling import process_logits
    R, step = 4, 40
    full, hist = _kernel_inputs(R, V, seed=V)
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=45, suppress_tokens=(0, 17, V - 1))
    want = process_logits(torch.log_softmax(full[:, :V], -1), hist, step, eos_token=EOS_K, **rules)
    x = full.to(dev)
    ops.logits_process(x[:, :V], torch.tensor([step, -1], dtype=torch.int32, device=dev), hist.to(dev), repetition_penalty=1.3,
                       no_repeat_ngram_size=2, min_new_tokens=45, eos=EOS_K,
                       suppress=torch.tensor([0, 17, V - 1], dtype=torch.int32, device=dev), normalize=True)
    got = x.cpu()
    assert torch.equal(_bits(got[:, V:]), _bits(full[:, V:]))
    banned = want == float("-inf")
    assert int(banned.sum()) > R * 4 and torch.equal(got[:, :V] == float("-inf"), banned)
    assert float((got[:, :V][~banned] - want[~banned]).abs().max()) <= 1e-5


@pytest.mark.parametrize("V", [1056, 50258])
@pytest.mark.parametrize("k", [1, 4])
def test_neutral_beam_form_then_normalized_topk_is_todays_topk(dev, V, k):
    from magma_amd import ops
    B = 2
    R = B * k
    g = torch.Generator().manual_seed(V + k)
    x = torch.zeros(R, V + 7, device=dev)
    x[:, :V] = (torch.randn(R, V, generator=g) * 4).to(dev)
    run = (torch.randn(R, generator=g) * 3 - 5).float()
    run.view(B, k)[0, 1:] = -1e9
    run = run.to(dev)
    cs, ct = torch.zeros(R, 2 * k, device=dev), torch.zeros(R, 2 * k, dtype=torch.int32, device=dev)
    ops.beam_topk(x[:, :V], run, cs, ct)
    y = x.clone()
    ops.logits_process(y[:, :V], torch.tensor([7, -1], dtype=torch.int32, device=dev), None, normalize=True)
    assert not torch.equal(y[:, :V], x[:, :V]) and torch.equal(y[:, V:], x[:, V:])
    cs2, ct2 = torch.zeros_like(cs), torch.zeros_like(ct)
    ops.beam_topk(y[:, :V], run, cs2, ct2, normalized=True)
    assert torch.equal(ct2, ct) and torch.equal(_bits(cs2), _bits(cs))


# ------------------------------------------------------------------------------------------------------- the reduced model
N = 12


def _rows(out, S, n, lengths=None):
    """The n generated ids of every row of generate()'s (B, S + n) output."""
    if lengths is None:
        return out[:, S:S + n].cpu()
    return torch.stack([out[b, int(s): int(s) + n].cpu() for b, s in enumerate(lengths)])


def _repeats(row, n):
    """Does the id list hold the same n-gram twice?"""
    grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
    return len(set(grams)) < len(grams)


def _violations(rows, rules, eos):
    """Which of the three properties the id rows break: a repeated n-gram, eos before min_new_tokens, a suppressed id."""
    rows = [r.tolist() if torch.is_tensor(r) else list(r) for r in rows]
    return dict(ngram=any(_repeats(r, rules["no_repeat_ngram_size"]) for r in rows),
                min_new=any(eos in r[: rules["min_new_tokens"]] for r in rows),
                suppress=any(t in rules["suppress_tokens"] for r in rows for t in r))


def _rules_from(plain, eos):
    """All four rules with values that bite on the plain run's rows: the n-gram size at which it repeats itself,
    min_new_tokens above its earliest eos, suppress ids taken from the tokens it emits."""
    rows = [r.tolist() for r in plain]
    n = 2 if any(_repeats(r, 2) for r in rows) else 1
    eos_at = [r.index(eos) for r in rows if eos in r[:-1]]
    assert eos_at, f"the plain run never emits eos before its last step: {rows}"
    emitted = [t for t in dict.fromkeys(t for r in rows for t in r) if t != eos]
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=n, min_new_tokens=min(eos_at) + 2,
                 suppress_tokens=tuple(emitted[:3]) or (eos,))
    assert all(_violations(rows, rules, eos).values()), (rules, rows)
    return rules


def _host_loop(model, emb, n, rules, lengths=None, select=None, past=None):
    """The host rule driven by the engine's own logits: prefill (or the new rows appended to ``past``), then eager decode steps
    fed the host's choice -- raw logits, host process_logits, then ``select`` (default argmax)."""
    from magma_amd.sampling import process_logits
    eng = model.lm.engine
    kw = {} if lengths is None else {"lengths": torch.as_tensor(lengths)}
    o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=n, past_key_values=past, **kw)
    c = o.past_key_values
    lg = o.logits[:, -1].float().cpu()
    hist = torch.zeros(emb.shape[0], n, dtype=torch.int64)
    for t in range(n):
        x = process_logits(lg, hist, t, eos_token=model.eos_token, **rules)
        hist[:, t] = x.argmax(-1) if select is None else select(x, t)
        if t + 1 < n:
            lg = eng.decode(hist[:, t:t + 1].to(model.device), c, use_graph=False)[0].float().cpu()
    return hist


def _gen(model, emb, n=N, lengths=None, **kw):
    kw.setdefault("temperature", 0.0)
    return model.generate(emb, max_steps=n, decode=False, stop_on_eos=False, lengths=lengths, **kw)


@pytest.mark.parametrize("cfg", ["v1", "ragged", "wide", "w8"])
def test_engine_greedy_equals_host_rule(dev, monkeypatch, cfg):
    kw = {"w8": dict(n_layer=1, n_head=16, d_ff=4096)}.get(cfg, {})
    model = _model(dev, monkeypatch, w8=cfg == "w8", **kw)
    assert model.lm.engine.decode_w8 == (cfg == "w8")
    B, S = (20 if cfg == "wide" else 3), 7
    emb = _emb(model, B, S, seed=40 + len(cfg))
    lengths = [7, 4, 5] if cfg == "ragged" else None
    plain = _rows(_gen(model, emb, lengths=lengths), S, N, lengths)
    assert torch.equal(plain, _host_loop(model, emb, N, {}, lengths))
    rules = _rules_from(plain, model.eos_token)
    got = _rows(_gen(model, emb, lengths=lengths, **rules), S, N, lengths)
    assert torch.equal(got, _host_loop(model, emb, N, rules, lengths)), (rules, got)
    assert not any(_violations(got, rules, model.eos_token).values()), (rules, got)


@pytest.mark.parametrize("cfg", ["v1", "ragged"])
def test_engine_beam_equals_host_rule(dev, cfg):
    from magma_amd.sampling import beam_search
    model = _model(dev)
    with torch.no_grad():       # a second favoured token beside eos: hypotheses that repeat it, then end (the captioning loop)
        model.lm.lm_head.bias[5] += 4.0
        model.lm.invalidate_packed()
    B, S, k = 3, 7, 4
    emb = _emb(model, B, S, seed=50 + len(cfg))
    lengths = [7, 4, 5] if cfg == "ragged" else None
    eng, eos = model.lm.engine, model.eos_token

    def host(rules):
        box = {}
        kw = {} if lengths is None else {"lengths": torch.as_tensor(lengths).repeat_interleave(k)}

        def step(rows, tokens):
            if rows is None:
                o = eng.forward(inputs_embeds=emb.repeat_interleave(k, dim=0), use_cache=True, cache_hint=N, **kw)
                box["c"] = o.past_key_values
                return o.logits[:, -1].float().cpu()
            c, r = box["c"], rows.to(dev)
            c.k.copy_(c.k.index_select(1, r))
            c.v.copy_(c.v.index_select(1, r))
            return eng.decode(tokens.view(-1, 1).to(dev), c, use_graph=False)[0].float().cpu()

        return beam_search(step, B, k, N, eos, 1.0, False, k, processors=rules or None)

    def device(rules):
        out, sc = model.generate(emb, max_steps=N, num_beams=k, num_return_sequences=k, decode=False, return_scores=True,
                                 lengths=lengths, **rules)
        return _rows(out, S, out.shape[1] - S, None if lengths is None else [x for x in lengths for _ in range(k)]), sc

    def hyps(seq, lens):          # every hypothesis up to its own length
        return [r[: int(m)].tolist() for r, m in zip(seq, lens)]

    p_seq, p_sc, p_len = host({})
    got, sc = device({})
    assert torch.equal(got, p_seq) and torch.allclose(sc, p_sc, rtol=1e-5, atol=1e-5)
    rows = hyps(p_seq, p_len)
    n = 2 if any(_repeats(r, 2) for r in rows) else 1
    assert int(p_len.min()) < N, "no plain hypothesis ends in eos before max_steps"
    emitted = [t for t in dict.fromkeys(t for r in rows for t in r) if t != eos]
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=n, min_new_tokens=min(max(int(p_len.min()) + 1, 4), N),
                 suppress_tokens=tuple(emitted[:3]))
    assert all(_violations(rows, rules, eos).values()), (rules, rows)
    r_seq, r_sc, r_len = host(rules)
    got, sc = device(rules)
    assert torch.equal(got, r_seq), (rules, got, r_seq)
    assert torch.allclose(sc, r_sc, rtol=1e-5, atol=1e-5), (sc, r_sc)
    assert not any(_violations(hyps(r_seq, r_len), rules, eos).values()), (rules, r_seq)


def test_engine_sampled_equals_host_rule(dev):
    """Fixed seed, temperature and top-k: the host loop draws with ops.sample from host-processed logits at the same seed and step."""
    from magma_amd import ops
    model = _model(dev)
    B, S, seed = 3, 7, 1234
    emb = _emb(model, B, S, seed=60)
    mode = dict(temperature=0.3, top_k=4, top_p=0.9)
    seed_d = torch.tensor([seed], dtype=torch.int64, device=dev)

    def draw(x, t):
        state = torch.tensor([t, -1], dtype=torch.int32, device=dev)
        return ops.sample(x.to(dev), mode["temperature"], mode["top_k"], mode["top_p"], seed_d, state).cpu()

    plain = _rows(_gen(model, emb, seed=seed, **mode), S, N)
    assert torch.equal(plain, _host_loop(model, emb, N, {}, select=draw))
    rules = _rules_from(plain, model.eos_token)
    got = _rows(_gen(model, emb, seed=seed, **mode, **rules), S, N)
    assert torch.equal(got, _host_loop(model, emb, N, rules, select=draw)), (rules, got)
    assert not any(_violations(got, rules, model.eos_token).values()), (rules, got)


def test_graph_replay_stale_values_and_the_default_path(dev, monkeypatch):
    from launch_trace import record
    from magma_amd import ops
    model = _model(dev)
    eng = model.lm.engine
    B, S = 3, 7
    emb = _emb(model, B, S, seed=70)
    plain = _rows(_gen(model, emb), S, N)
    rules = _rules_from(plain, model.eos_token)
    ref = _host_loop(model, emb, N, rules)
    a = _rows(_gen(model, emb, **rules), S, N)          # eager first step, captures the second, replays the rest
    b = _rows(_gen(model, emb, **rules), S, N)          # replays every step
    assert torch.equal(a, ref) and torch.equal(b, ref)
    graphs = next(iter(eng._cache_pool.values())).decode_state.graphs
    n_graphs = len(graphs)
    orig = eng.decode
    monkeypatch.setattr(eng, "decode", lambda *x, **kw: orig(*x, **{**kw, "use_graph": False}))
    assert torch.equal(_rows(_gen(model, emb, **rules), S, N), ref)
    monkeypatch.undo()
    # other values on the same cache: that call's host result, and a step captured under its own key
    other = dict(rules, repetition_penalty=2.5, no_repeat_ngram_size=3 - rules["no_repeat_ngram_size"],
                 min_new_tokens=rules["min_new_tokens"] + 1, suppress_tokens=rules["suppress_tokens"][:1])
    assert torch.equal(_rows(_gen(model, emb, **other), S, N), _host_loop(model, emb, N, other))
    assert len(graphs) == n_graphs + 1
    # the same count of suppress ids, other ids: the captured step is replayed and reads the new ones
    swapped = dict(rules, suppress_tokens=tuple(int(t) for t in ref[0, :len(rules["suppress_tokens"])]))
    n_graphs = len(graphs)
    assert torch.equal(_rows(_gen(model, emb, **swapped), S, N), _host_loop(model, emb, N, swapped))
    assert len(graphs) == n_graphs
    assert torch.equal(_rows(_gen(model, emb), S, N), plain)
    # the four defaults: the plain call's bits and the plain call's launches, no processor launch among them
    calls = []
    real = ops.logits_process
    monkeypatch.setattr(ops, "logits_process", lambda *x, **kw: (calls.append(1), real(*x, **kw))[1])
    monkeypatch.setattr(eng, "decode", lambda *x, **kw: orig(*x, **{**kw, "use_graph": False}))
    neutral = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=None)
    for extra in (dict(), dict(num_beams=2), dict(temperature=0.7, top_k=5, seed=3)):
        rec_a, out_a = record(eng, lambda: _gen(model, emb, 5, **extra))
        rec_b, out_b = record(eng, lambda: _gen(model, emb, 5, **extra, **neutral))
        assert not isinstance(out_a, Exception) and not isinstance(out_b, Exception), (out_a, out_b)
        assert torch.equal(out_a, out_b) and rec_a == rec_b and len(rec_a) > 20
    assert not calls
    rec_p, _ = record(eng, lambda: _gen(model, emb, 5))
    rec_c, _ = record(eng, lambda: _gen(model, emb, 5, **rules))
    assert len(calls) == 5 and [r["op"] for r in rec_c] == [r["op"] for r in rec_p]      # one processor launch per token, nothing else


def test_continued_cache_rules_cover_the_current_call_only(dev):
    model = _model(dev)
    B, S, T = 3, 7, 4
    emb, q = _emb(model, B, S, seed=80), _emb(model, B, T, seed=81)
    turn1 = [model.generate(emb, max_steps=6, temperature=0.0, decode=False, return_past_key_values=True) for _ in range(2)]
    assert torch.equal(turn1[0][0], turn1[1][0])
    (_, past_a), (_, past_b) = turn1
    past_c = model.generate(emb, max_steps=6, temperature=0.0, decode=False, return_past_key_values=True)[1]
    plain = _rows(_gen(model, q, past_key_values=past_c), T, N)
    rules = dict(repetition_penalty=2.5)
    got = _rows(_gen(model, q, past_key_values=past_a, **rules), T, N)
    ref = _host_loop(model, q, N, rules, past=past_b)          # the host history holds turn 2's tokens only
    assert torch.equal(got, ref), (got, ref)
    assert not torch.equal(got, plain), "the penalty left turn 2 as it was"


def test_full_width_vocabulary(dev):
    """d = 4096, V = 50 258, one block, B = 2, 6 steps, all four rules inside the captured step."""
    model = _model(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=128)
    emb = _emb(model, 2, 5, seed=90)
    plain = _rows(_gen(model, emb, 6), 5, 6)
    first = [int(t) for t in plain[:, 0]]
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=1, min_new_tokens=6, suppress_tokens=tuple(dict.fromkeys(first)))
    got = _rows(_gen(model, emb, 6, **rules), 5, 6)
    assert torch.equal(got, _host_loop(model, emb, 6, rules)), got
    assert not any(_violations(got, rules, model.eos_token).values()) and not torch.equal(got, plain)
