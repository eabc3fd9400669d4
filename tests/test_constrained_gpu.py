"""Constrained decoding on the device (DESIGN.md "Constrained decoding"): the kernel against the host rule
(magma_amd.sampling.constrain_logits, pinned to transformers by tests/test_constrained_cpu.py) value for value, its path cache
against fresh buffers, and generate(constraint=...) / Magma.choose on the reduced model -- greedy, both samplers, per-row
stopping, log-probabilities, a continued cache, captured steps -- against the host rule driven by the engine's own decode logits."""
import pytest
import torch

from test_beam_search_gpu import _emb, _model

pytestmark = pytest.mark.gpu

HC = 66                     # history columns of the kernel tests: one 64-token sequence, its eos and one pad
N = 8


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ the kernel
_TRIES = {}


def _tries(V):
    """(A, B, s64): A holds a root with min(V, 3100) - 2 edges (more than the workgroup has threads from V = 1056 on), edge tokens
    0 and V - 1, the terminal inner node [5, 6] under [5, 6, 9], and a 64-token sequence; B is a root with one edge."""
    from magma_amd.sampling import TokenTrie
    if V not in _TRIES:
        s64 = [0, V - 1] + [2 + (i * 7) % min(V - 2, 29) for i in range(62)]
        singles = [[t] for t in range(1, min(V, 3100)) if t != 5]
        a = TokenTrie(singles + [[V - 1], s64, [5, 6], [5, 6, 9], [5, 11]])
        assert a.first[1] - a.first[0] >= min(V, 3100) - 2 and a.max_len() == 64
        _TRIES[V] = (a, TokenTrie([[7, 8]]), s64)
    return _TRIES[V]


def _tracks(V, s64, eos):
    """Histories [7, HC]: the 64-token sequence then eos; a leaf then eos; eos at a terminal inner node; off the trie at the
    second token, followed by tokens that are edges of the root; B's sequence; the edge V - 1; the last edge of A's root."""
    pad = [eos] * HC
    rows = [s64 + pad, [5, 6, 9] + pad, [5, 6] + pad, [5, 4, 5, 6, 9, 5, 6] + pad, [7, 8] + pad, [V - 1] + pad,
            [min(V, 3100) - 1, 0, V - 1] + pad]
    return torch.tensor([r[:HC] for r in rows], dtype=torch.int64)


STEPS = [0, 1, 2, 3, 4, 63, 64, 65, HC, HC + 4]       # root, inner, terminal inner / off, leaf, after eos, deep, == and > history_cols


def _case(R, V, seed, eos):
    """(logits [R, V + 7] with a sentinel in the padding, histories [R, HC], one trie per row)."""
    a, b, s64 = _tries(V)
    g = torch.Generator().manual_seed(seed)
    full = torch.full((R, V + 7), 123.25)
    full[:, :V] = torch.randn(R, V, generator=g) * 3
    full[:, 0], full[:, V - 1], full[:, 5] = 0.5, float("-inf"), -0.0
    tr = _tracks(V, s64, eos)
    hist = torch.stack([tr[(r * 3 + seed) % len(tr)] for r in range(R)])
    tries = [b if r % 4 == 3 else a for r in range(R)]
    return full, hist, tries


def _want(full, V, hist, step, tries, eos_ids, rules=None):
    from magma_amd.sampling import constrain_logits, process_logits
    n = min(step, hist.shape[1])
    x = full[:, :V]
    if rules:
        x = process_logits(x, hist, n, eos_token=list(eos_ids), **rules)
    want = full.clone()
    want[:, :V] = constrain_logits(x, hist, n, tries, eos_ids)
    return want


def _launch(dev, full, V, hist_d, step, bufs, eos_ids, rules=None):
    from magma_amd import ops
    table, roots, path = bufs
    x = full.to(dev)
    kw = {}
    if rules:
        kw = dict(repetition_penalty=rules["repetition_penalty"], min_new_tokens=rules["min_new_tokens"],
                  suppress=torch.tensor(rules["suppress_tokens"], dtype=torch.int32, device=dev))
    if len(eos_ids) > 1:
        kw["eos_more"] = torch.tensor(eos_ids[1:], dtype=torch.int32, device=dev)
    ops.logits_process_constrained(x[:, :V], torch.tensor([step, -1], dtype=torch.int32, device=dev), hist_d, table, roots, path,
                                   eos=eos_ids[0], **kw)
    return x.cpu()


def _bufs(dev, tries, spare=0):
    from magma_amd import ops
    from magma_amd.sampling import trie_forest
    table, roots = trie_forest(tries)
    buf = torch.zeros(table.numel() + spare, dtype=torch.int32)
    buf[: table.numel()] = table
    return buf.to(dev), roots.to(dev), ops.trie_path(len(tries), dev)


@pytest.mark.parametrize("V", [33, 1056, 50258])
@pytest.mark.parametrize("R", [1, 3, 17])
def test_kernel_is_the_host_rule_value_for_value(dev, R, V):
    on_trie = 0
    for eos_ids in ((3,), (3, 4, V - 2)):
        full, hist, tries = _case(R, V, seed=len(eos_ids) - 1, eos=eos_ids[0])      # row 0 walks the 64-token sequence, then [5, 6]
        bufs, hist_d = _bufs(dev, tries, spare=5), hist.to(dev)
        for step in STEPS:
            want = _want(full, V, hist, step, tries, eos_ids)
            got = _launch(dev, full, V, hist_d, step, bufs, eos_ids)
            assert torch.equal(_bits(got), _bits(want)), (eos_ids, step, (_bits(got) != _bits(want)).nonzero()[:8])
            on_trie += sum(t.node(h[: min(step, HC)].tolist()) is not None for t, h in zip(tries, hist))
    assert on_trie >= 8          # the walks stay on the trie at several steps


def test_kernel_path_cache_is_invisible(dev):
    """Steps out of order, another trie and other histories in between, garbage in the cache: the results of fresh buffers."""
    R, V, eos_ids = 5, 1056, (3, 4)
    full, hist, tries = _case(R, V, seed=2, eos=3)
    a, b, _ = _tries(V)
    other_tries = [b, a, a, b, a]
    other_hist = hist.roll(2, 0).contiguous()
    used = _bufs(dev, tries, spare=64)
    other = _bufs(dev, other_tries)
    n_other = other[0].numel()
    assert n_other <= used[0].numel()
    for step in [64, 3, 65, 0, 2, 63, 1, HC, 4, 2, 64]:
        want = _want(full, V, hist, step, tries, eos_ids)
        fresh = _launch(dev, full, V, hist.to(dev), step, _bufs(dev, tries), eos_ids)
        got = _launch(dev, full, V, hist.to(dev), step, used, eos_ids)
        assert torch.equal(_bits(fresh), _bits(want)) and torch.equal(_bits(got), _bits(want)), step
        # the same buffers serve another trie (other roots, other node numbers) and other histories, at the next step
        table, roots, path = used
        saved = table.clone(), roots.clone()
        table[:n_other].copy_(other[0])
        roots.copy_(other[1])
        got = _launch(dev, full, V, other_hist.to(dev), step + 1, used, eos_ids)
        assert torch.equal(_bits(got), _bits(_want(full, V, other_hist, step + 1, other_tries, eos_ids))), step
        table.copy_(saved[0])
        roots.copy_(saved[1])
    # a cache of arbitrary numbers, node ids in and out of range
    g = torch.Generator().manual_seed(0)
    used[2].copy_(torch.randint(-5, 4000, used[2].shape, generator=g).to(torch.int32))
    for step in (64, 2):
        assert torch.equal(_bits(_launch(dev, full, V, hist.to(dev), step, used, eos_ids)),
                           _bits(_want(full, V, hist, step, tries, eos_ids)))
    # a table that is none (counts beyond the buffer): off the trie for every row, nothing outside the buffer is read
    bad = (torch.tensor([10 ** 6, 10 ** 6, 0, 0], dtype=torch.int32, device=dev), used[1], used[2])
    got = _launch(dev, full, V, hist.to(dev), 1, bad, eos_ids)
    assert bool((got[:, list(eos_ids)] == full[:, list(eos_ids)]).all()) and int((got[:, :V] > float("-inf")).sum()) == R * 2


@pytest.mark.parametrize("V", [1056, 50258])
def test_kernel_with_the_other_rules_in_one_launch(dev, V):
    R, eos_ids = 3, (3, 4)
    full, hist, tries = _case(R, V, seed=7, eos=3)
    rules = dict(repetition_penalty=1.3, min_new_tokens=3, suppress_tokens=(2, 6, V - 1))
    bufs, hist_d = _bufs(dev, tries), hist.to(dev)
    differs = 0
    for step in (0, 1, 2, 3, 64, HC):
        want = _want(full, V, hist, step, tries, eos_ids, rules)
        got = _launch(dev, full, V, hist_d, step, bufs, eos_ids, rules)
        assert torch.equal(_bits(got), _bits(want)), (step, (_bits(got) != _bits(want)).nonzero()[:8])
        differs += int(not torch.equal(_bits(want), _bits(_want(full, V, hist, step, tries, eos_ids))))
    assert differs >= 3          # the penalty, the eos ban or the suppress list changed a kept column


# ------------------------------------------------------------------------------------------------------- the reduced model
def _rows(out, S, n, lengths=None):
    if lengths is None:
        return out[:, S:S + n].cpu()
    return torch.stack([out[b, int(s): int(s) + n].cpu() for b, s in enumerate(lengths)])


def _gen(model, emb, n=N, lengths=None, **kw):
    kw.setdefault("temperature", 0.0)
    return model.generate(emb, max_steps=n, decode=False, stop_on_eos=False, lengths=lengths, **kw)


def _host_loop(model, emb, n, tries, rules=None, lengths=None, select=None, past=None, eos_ids=None):
    """The host rule driven by the engine's own logits: prefill (or the new rows appended to ``past``), then eager decode steps
    fed the host's choice -- raw logits, host process_logits and constrain_logits, then ``select`` (default argmax)."""
    from magma_amd.sampling import TokenTrie, constrain_logits, process_logits
    eng = model.lm.engine
    per_row = eos_ids is not None               # per-row stopping: a finished row is padded with the first eos id
    eos_ids = eos_ids or (model.eos_token,)
    kw = {} if lengths is None else {"lengths": torch.as_tensor(lengths)}
    o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=n, past_key_values=past, **kw)
    c = o.past_key_values
    lg = o.logits[:, -1].float().cpu()
    B = emb.shape[0]
    tries = [tries] * B if isinstance(tries, TokenTrie) else tries
    hist = torch.zeros(B, n, dtype=torch.int64)
    done = torch.zeros(B, dtype=torch.bool)
    for t in range(n):
        x = process_logits(lg, hist, t, eos_token=list(eos_ids), **rules) if rules else lg
        x = constrain_logits(x, hist, t, tries, eos_ids)
        tok = x.argmax(-1) if select is None else select(x, t)
        hist[:, t] = torch.where(done, torch.full_like(tok, eos_ids[0]), tok)
        done |= torch.isin(hist[:, t], torch.tensor(list(eos_ids))) & per_row
        if t + 1 < n:
            lg = eng.decode(hist[:, t:t + 1].to(model.device), c, use_graph=False)[0].float().cpu()
    return hist


def _listed(row, trie, eos):
    row = row.tolist()
    n = row.index(eos) if eos in row else len(row)
    return trie.index(row[:n]) >= 0 and all(t == eos for t in row[n:])


def _choices(plain, eos, V, seed=0, count=6):
    """Sequences of 1 to 4 ids, none starting with a token the plain run starts with; one is a prefix of another."""
    first = {int(t) for t in plain[:, 0]} | {eos}
    g = torch.Generator().manual_seed(seed)
    free = [t for t in torch.randperm(V, generator=g).tolist() if t not in first]
    seqs = [free[4 * i: 4 * i + 1 + i % 4] for i in range(count)]
    return seqs + [seqs[min(3, count - 1)][:2]]


@pytest.mark.parametrize("cfg", ["v1", "ragged", "wide", "w8"])
def test_engine_greedy_equals_host_rule(dev, monkeypatch, cfg):
    from magma_amd.sampling import TokenTrie
    kw = {"w8": dict(n_layer=1, n_head=16, d_ff=4096)}.get(cfg, {})
    model = _model(dev, monkeypatch, w8=cfg == "w8", **kw)
    assert model.lm.engine.decode_w8 == (cfg == "w8")
    B, S = (20 if cfg == "wide" else 3), 7
    eos, V = model.eos_token, model.lm.engine.V
    emb = _emb(model, B, S, seed=40 + len(cfg))
    lengths = [7, 4, 5] if cfg == "ragged" else None
    plain = _rows(_gen(model, emb, lengths=lengths), S, N, lengths)
    trie = TokenTrie(_choices(plain, eos, V))
    assert not any(_listed(r, trie, eos) for r in plain)
    got = _rows(_gen(model, emb, lengths=lengths, constraint=trie), S, N, lengths)
    assert torch.equal(got, _host_loop(model, emb, N, trie, lengths=lengths)), got
    assert all(_listed(r, trie, eos) for r in got), got
    # one trie per row (multiple choice), given as lists
    rows = [_choices(plain, eos, V, seed=1 + b % 3, count=3 + b % 3) for b in range(B)]
    got = _rows(_gen(model, emb, lengths=lengths, constraint=rows), S, N, lengths)
    tries = [TokenTrie(r) for r in rows]
    assert torch.equal(got, _host_loop(model, emb, N, tries, lengths=lengths)), got
    assert all(_listed(r, t, eos) for r, t in zip(got, tries)), got


@pytest.mark.parametrize("sampler", ["reference", "transformers"])
def test_engine_sampled_equals_host_rule(dev, sampler):
    from magma_amd import ops
    from magma_amd.sampling import TokenTrie
    model = _model(dev)
    B, S, seed = 3, 7, 1234
    emb = _emb(model, B, S, seed=60)
    eos, V = model.eos_token, model.lm.engine.V
    mode = dict(temperature=1.3, top_k=4, top_p=0.9)
    if sampler == "transformers":
        mode.update(sampler=sampler, min_p=0.02)
    seed_d = torch.tensor([seed], dtype=torch.int64, device=dev)

    def draw(x, t):
        state = torch.tensor([t, -1], dtype=torch.int32, device=dev)
        if sampler == "transformers":
            return ops.sample_warp(x.to(dev), mode["temperature"], mode["top_k"], mode["top_p"], mode["min_p"], seed_d, state).cpu()
        return ops.sample(x.to(dev), mode["temperature"], mode["top_k"], mode["top_p"], seed_d, state).cpu()

    plain = _rows(_gen(model, emb, seed=seed, **mode), S, N)
    trie = TokenTrie(_choices(plain, eos, V, count=12))
    got = _rows(_gen(model, emb, seed=seed, constraint=trie, **mode), S, N)
    assert torch.equal(got, _host_loop(model, emb, N, trie, select=draw)), got
    assert all(_listed(r, trie, eos) for r in got) and not any(_listed(r, trie, eos) for r in plain)


def test_per_row_stopping_logprobs_and_rules(dev):
    from magma_amd.sampling import TokenTrie
    from test_logprobs_gpu import _check_against, _replay
    model = _model(dev)
    B, S = 3, 7
    emb = _emb(model, B, S, seed=65)
    eos, V = model.eos_token, model.lm.engine.V
    plain = _rows(_gen(model, emb), S, N)
    seqs = _choices(plain, eos, V)
    eos_ids = [eos, seqs[0][0]]                 # a second eos id (a token of no row's trie)
    rows = [[seqs[1]], [seqs[2]], [seqs[3]]]    # one choice per row, of 2, 3 and 4 tokens
    out, fin = model.generate(emb, max_steps=N, temperature=0.0, decode=False, eos_token=eos_ids, return_finish=True, constraint=rows)
    assert fin.reason == ["eos"] * B and fin.kept.tolist() == [3, 4, 5] and out.shape[1] == S + 5
    for b in range(B):
        assert out[b, S: S + len(rows[b][0])].tolist() == rows[b][0] and int(out[b, S + len(rows[b][0])]) in eos_ids
    assert torch.equal(out[:, S:].cpu(), _host_loop(model, emb, 5, [TokenTrie(r) for r in rows], eos_ids=eos_ids))
    # log-probabilities: of the raw distribution, whatever the constraint and the penalty did to the copy
    trie = TokenTrie(seqs)
    spare = next(t for t in range(V) if t != eos and t not in trie.tokens())      # (a suppress id may meet neither the trie nor eos)
    for rules in ({}, dict(repetition_penalty=1.7, min_new_tokens=1, suppress_tokens=[spare])):
        out, lps = _gen(model, emb, constraint=trie, return_logprobs=True, top_logprobs=3, **rules)
        got = _rows(out, S, N)
        assert torch.equal(got, _host_loop(model, emb, N, trie, rules=rules)) and all(_listed(r, trie, eos) for r in got)
        assert torch.equal(lps.tokens, got)
        _check_against(lps, _replay(model, emb, lps.tokens), V, f"constraint {sorted(rules)}")
        assert float(lps.logprobs.max()) < 0.0


def test_continued_cache_starts_at_the_root_again(dev):
    from magma_amd.sampling import TokenTrie
    model = _model(dev)
    B, S, T = 3, 7, 4
    emb, q = _emb(model, B, S, seed=80), _emb(model, B, T, seed=81)
    eos, V = model.eos_token, model.lm.engine.V
    pasts = [model.generate(emb, max_steps=6, temperature=0.0, decode=False, return_past_key_values=True)[1] for _ in range(3)]
    plain = _rows(_gen(model, q, past_key_values=pasts[2]), T, N)
    trie = TokenTrie(_choices(plain, eos, V))
    got = _rows(_gen(model, q, past_key_values=pasts[0], constraint=trie), T, N)
    assert torch.equal(got, _host_loop(model, q, N, trie, past=pasts[1])), got          # the host history holds turn 2's tokens only
    assert all(_listed(r, trie, eos) for r in got) and not any(_listed(r, trie, eos) for r in plain)


def test_graph_replay_other_tries_and_the_default_path(dev, monkeypatch):
    from launch_trace import OPS, record
    from magma_amd import ops
    from magma_amd.sampling import TokenTrie
    model = _model(dev)
    eng = model.lm.engine
    B, S = 3, 7
    emb = _emb(model, B, S, seed=70)
    eos, V = model.eos_token, eng.V
    plain = _rows(_gen(model, emb), S, N)
    trie = TokenTrie(_choices(plain, eos, V))
    ref = _host_loop(model, emb, N, trie)
    a = _rows(_gen(model, emb, constraint=trie), S, N)          # eager first step, captures the second, replays the rest
    b = _rows(_gen(model, emb, constraint=trie), S, N)          # replays every step
    assert torch.equal(a, ref) and torch.equal(b, ref)
    cache = next(iter(eng._cache_pool.values()))
    graphs = cache.decode_state.graphs
    n_graphs, table = len(graphs), cache.trie_table
    # other tries that fit the buffer, smaller and larger, shared and per row: the captured steps, that trie's host result
    small = TokenTrie(_choices(plain, eos, V, seed=9, count=1))
    large = TokenTrie(_choices(plain, eos, V, seed=5, count=150))
    per_row = [trie, small, large]
    for t in (small, large, per_row, trie):
        got = _rows(_gen(model, emb, constraint=t), S, N)
        assert torch.equal(got, _host_loop(model, emb, N, t)), got
        assert len(graphs) == n_graphs and cache.trie_table is table
    # a table that outgrows the buffer: a new buffer, the steps captured on the old one dropped and captured again
    huge = TokenTrie([[t] for t in range(V) if t != eos] + [[t, 5] for t in range(0, V, 7) if t != eos])
    assert huge.flat().numel() > table.numel()
    got = _rows(_gen(model, emb, constraint=huge), S, N)
    assert torch.equal(got, _host_loop(model, emb, N, huge)) and cache.trie_table is not table and len(graphs) == n_graphs
    assert torch.equal(_rows(_gen(model, emb, constraint=trie), S, N), ref)
    assert torch.equal(_rows(_gen(model, emb), S, N), plain)
    # constraint=None: the plain call's bits and the plain call's launches, no processor launch among them
    calls = []
    orig = eng.decode
    monkeypatch.setattr(eng, "decode", lambda *x, **kw: orig(*x, **{**kw, "use_graph": False}))
    with monkeypatch.context() as m:
        for name in ("logits_process", "logits_process_constrained"):
            m.setattr(ops, name, lambda *x, _real=getattr(ops, name), **kw: (calls.append(1), _real(*x, **kw))[1])
        for extra in (dict(), dict(num_beams=2), dict(temperature=0.7, top_k=5, seed=3)):
            rec_a, out_a = record(eng, lambda: _gen(model, emb, 5, **extra))
            rec_b, out_b = record(eng, lambda: _gen(model, emb, 5, constraint=None, **extra))
            assert not isinstance(out_a, Exception) and not isinstance(out_b, Exception), (out_a, out_b)
            assert torch.equal(out_a, out_b) and rec_a == rec_b and len(rec_a) > 20
        assert not calls
    # a constraint alone: the plain launches plus one processor launch per token; with the other rules: their launches
    names = OPS + ("logits_process", "logits_process_constrained")

    def ops_of(fn):
        recs, res = record(eng, fn, op_names=names)
        assert not isinstance(res, Exception), res
        return [r["op"] for r in recs]

    plain_ops = ops_of(lambda: _gen(model, emb, 5))
    cons_ops = ops_of(lambda: _gen(model, emb, 5, constraint=trie))
    assert cons_ops.count("logits_process_constrained") == 5 and "logits_process" not in cons_ops
    assert [o for o in cons_ops if o != "logits_process_constrained"] == plain_ops
    at = [i for i, o in enumerate(cons_ops) if o == "logits_process_constrained"]
    assert all(cons_ops[i + 1] == "argmax" for i in at)            # in front of the selection
    rules = dict(repetition_penalty=1.3, min_new_tokens=1, suppress_tokens=[next(t for t in range(V) if t != eos and t not in trie.tokens())])
    rule_ops = ops_of(lambda: _gen(model, emb, 5, **rules))
    both_ops = ops_of(lambda: _gen(model, emb, 5, constraint=trie, **rules))
    assert rule_ops.count("logits_process") == 5 and [o.replace("_constrained", "") for o in both_ops] == rule_ops


def test_full_width_vocabulary(dev):
    """d = 4096, V = 50 258, one block, B = 2, 6 steps, a trie of a few hundred sequences inside the captured step."""
    from magma_amd.sampling import TokenTrie
    model = _model(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=128)
    emb = _emb(model, 2, 5, seed=90)
    eos = model.eos_token
    plain = _rows(_gen(model, emb, 6), 5, 6)
    trie = TokenTrie(_choices(plain, eos, 50258, count=300))
    got = _rows(_gen(model, emb, 6, constraint=trie), 5, 6)
    assert torch.equal(got, _host_loop(model, emb, 6, trie)), got
    assert all(_listed(r, trie, eos) for r in got) and not any(_listed(r, trie, eos) for r in plain)


def test_choose_on_the_engine(dev):
    from magma_amd.sampling import TokenTrie
    model = _model(dev)
    B, S = 3, 7
    emb = _emb(model, B, S, seed=95)
    eos, V = model.eos_token, model.lm.engine.V
    plain = _rows(_gen(model, emb), S, N)
    rows = [_choices(plain, eos, V, seed=b, count=4 + b) for b in range(B)]
    tries = [TokenTrie(r) for r in rows]
    index, lps = model.choose(emb, rows)
    n = max(t.max_len() for t in tries) + 1
    host = _host_loop(model, emb, n, tries)
    want = [t.index(r.tolist()[: r.tolist().index(eos)]) for r, t in zip(host, tries)]
    assert index.tolist() == want and min(want) >= 0
    assert all(int(c) <= len(rows[b][i]) + 1 for b, (c, i) in enumerate(zip(lps.count, want)))
    assert lps.count.tolist() == [len(rows[b][i]) + 1 for b, i in enumerate(want)]
    shared, _ = model.choose(emb, rows[0])
    assert int(shared[0]) == want[0]
