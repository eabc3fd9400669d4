"""transformers' sampler on the device (csrc/sampling.hip, the WARP instance of sample_kernel; DESIGN.md "transformers'
sampler"): ops.sample_warp and generate(sampler="transformers").

  * the kept sets against the host statements (magma_amd/sampling.py warp_filter -- themselves equal to transformers' chained
    warpers, tests/test_nucleus_sampling_cpu.py) and against transformers' own masks pinned in tests/golden/warper_pins.pt.
    Bounds: the device evaluates exp in fp32 (__expf), the host in float64, so the nucleus boundary may move by one rank: on
    tie-free rows at most ONE differing element per row; on tied rows the differences lie among equal values only and the
    number of survivors per distinct value is off by at most 1 in total;
  * the draw against the float64 restatement of the Philox stream, and its frequencies against the renormalised nucleus;
  * generate(): reproducibility, captured graph == eager launches, the degenerate settings that must equal greedy decoding,
    the combinations with processors / stopping / ragged batches / continued caches, and the untouched defaults."""
import os

import numpy as np
import pytest
import torch

import warper_cases as W

pytestmark = pytest.mark.gpu

PINS = torch.load(os.path.join(os.path.dirname(__file__), "golden", "warper_pins.pt"), weights_only=False)


def _filter(x, temperature, top_k, top_p, min_p):
    from magma_amd import ops
    xd = x.cuda().float().contiguous()
    f = torch.empty_like(xd)
    ops.sample_warp(xd, temperature, top_k, top_p, min_p, None, None, filtered=f, want_token=False)
    return f.cpu()


def _check_sets(x, got, want_kept, tie_free, what):
    """``got``: the device's filtered logits; ``want_kept``: the mask it is held against."""
    kept = ~torch.isneginf(got)
    assert bool((torch.isneginf(got) | (got == x)).all()), what                       # only -inf or the original value
    assert bool(kept.gather(1, x.argmax(1, keepdim=True)).all()), what                # the first maximum is never dropped
    assert not bool((kept & torch.isneginf(x)).any()), what
    for r in range(x.shape[0]):
        if tie_free:
            n = int((kept[r] != want_kept[r]).sum())
            assert n <= 1, (what, r, n)
        else:
            n = W.count_diff(x[r], kept[r], want_kept[r])
            assert n <= 1, (what, r, n)
    return kept


@pytest.mark.parametrize("V", [50258, 1000, 65, 1])
@pytest.mark.parametrize("kind", W.KINDS)
def test_filter_sets_device_vs_host_statement(dev, kind, V):
    x = W.make_rows(kind, 6, V)
    fired = 0
    for prm in W.GRID:
        got = _filter(x, *prm)
        kept = _check_sets(x, got, W.host_kept(x, *prm), kind in W.TIE_FREE, (kind, V, prm))
        fired += int((~kept).any())
    if V >= 1000:
        assert fired >= len(W.GRID) // 2          # the rules dropped something in most settings
    if kind == "peaked" and V == 50258:           # where the reference's rule is a no-op (test_sampling_gpu.py), this one is not
        assert int((~torch.isneginf(_filter(x, 1.0, 0, 0.9, 0.0))).sum(1).max()) < 10


def test_filter_sets_device_vs_transformers_pins(dev):
    x, nt = PINS["logits"], PINS["tie_free_rows"]
    want = W.unpack(PINS["kept"], x.shape[1])
    for i, prm in enumerate(PINS["params"]):
        got = _filter(x, *prm)
        _check_sets(x[:nt], got[:nt], want[i, :nt], True, ("pins", prm))
        _check_sets(x[nt:], got[nt:], want[i, nt:], False, ("pins", prm))


@pytest.mark.parametrize("V", [50258, 1000])
def test_rows_with_banned_entries(dev, V):
    """-inf entries (processor bans) carry no mass, stay -inf and are never selected -- also when all but one are banned."""
    from magma_amd import ops
    x = W.make_rows("randn3", 6, V)
    g = torch.Generator().manual_seed(9)
    x[:4] = x[:4].masked_fill(torch.rand(4, V, generator=g) < 0.25, float("-inf"))
    x[4:] = float("-inf")
    x[4, V - 1], x[5, 0] = 0.5, -3.0
    seed = torch.tensor([5], dtype=torch.int64, device=dev)
    state = torch.tensor([3, -1], dtype=torch.int32, device=dev)
    for prm in ((0.7, 0, 0.9, 0.0), (1.3, 40, 0.3, 0.05), (1.0, 0, 0.0, 0.05), (0.7, 1000, 1.0, 0.0), (1.0, 0, 1e-6, 0.0)):
        f = torch.empty(6, V, device=dev)
        tok = ops.sample_warp(x.to(dev), *prm, seed, state, filtered=f).cpu()
        kept = _check_sets(x, f.cpu(), W.host_kept(x, *prm), True, (V, prm))
        assert bool(kept.gather(1, tok[:, None]).all()), (V, prm, tok)
        assert kept[4].nonzero().tolist() == [[V - 1]] and kept[5].nonzero().tolist() == [[0]]
        assert tok[4:].tolist() == [V - 1, 0]


@pytest.mark.parametrize("V", [50258, 20])
def test_top_k_keeps_every_tie_at_the_kth_value(dev, V):
    """Five equal values straddle k: transformers' rule keeps them all (the reference's keeps exactly k: test_sampling_gpu.py)."""
    from magma_amd import sampling as S
    x = -torch.arange(float(V))[None, :].repeat(2, 1)              # descending, all distinct
    ties = [3, 7, V // 2, V - 2, V - 1]
    x[:, ties] = -5.0                                               # 0 -1 -2 -4 above, then -5 six times (index 5 holds it too): ranks 4 .. 9
    x[1] = x[1].flip(0)
    for k in (5, 7, 10):
        got = _filter(x, 1.0, k, 0.0, 0.0)
        want = S.top_k_filter_ties(x, k)
        assert torch.equal(got, want), k
        assert (~torch.isneginf(got)).sum(1).tolist() == [10, 10]  # four values above and all six ties
    assert (~torch.isneginf(_filter(x, 1.0, 4, 0.0, 0.0))).sum(1).tolist() == [4, 4]
    assert (~torch.isneginf(_filter(x, 1.0, 11, 0.0, 0.0))).sum(1).tolist() == [11, 11]


# ---- the draw: the float64 statement of tests/test_sampling_gpu.py, restated here (that module must not change) ----
def philox4x32_10(c, k0, k1):
    c = [int(v) & 0xFFFFFFFF for v in c]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def restated_draw(row, kept, temperature, seed, step, b):
    """float64 statement of the draw: u = 64 Philox bits / 2^64, first index whose inclusive CDF exceeds u * total."""
    c = philox4x32_10([step, b, 0, 0], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = ((c[0] << 32) | c[1]) / 2.0 ** 64
    x = row.double().numpy()
    w = np.where(kept.numpy(), np.exp((x - x.max()) / temperature), 0.0)
    cdf = np.cumsum(w)
    t = u * cdf[-1]
    i = int(np.searchsorted(cdf, t, side="right"))
    margin = min(abs(t - cdf[i - 1]) if i > 0 else 1.0, abs(cdf[i] - t)) / cdf[-1]
    return i, margin


def test_multinomial_matches_restatement(dev):
    from magma_amd import ops
    V, B = 50258, 8
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, V, generator=g) * 3.0)
    xs = x.cuda()
    seed = 0x1234_5678_9ABC_DEF1
    seed_t = torch.tensor([seed], dtype=torch.int64, device="cuda")
    for (T, k, p, mp) in ((0.7, 0, 0.9, 0.0), (1.3, 50, 0.5, 0.0), (1.0, 0, 0.0, 0.05)):
        f = torch.empty_like(xs)
        for step in (0, 1, 5, 1000):
            state = torch.tensor([step, -1], dtype=torch.int32, device="cuda")
            tok = ops.sample_warp(xs, T, k, p, mp, seed_t, state, filtered=f).cpu()
            kept = ~torch.isneginf(f.cpu())
            assert 1 <= int(kept.sum(1).min()) and int(kept.sum(1).max()) < V // 4
            for b in range(B):
                want, margin = restated_draw(x[b], kept[b], T, seed, step, b)
                assert bool(kept[b, tok[b]])
                assert int(tok[b]) == want or margin < 1e-6, (T, k, p, mp, step, b, int(tok[b]), want, margin)


def test_multinomial_frequencies_of_the_nucleus(dev):
    """4000 draws (4000 rows) from one 6-way distribution at top_p = 0.8: the nucleus is its two most probable tokens
    (0.629 + 0.180; the four others sum to 0.1905 <= 0.2), drawn within 4.5 sigma of their renormalised probabilities; the
    dropped tokens are never drawn."""
    from magma_amd import ops
    V, N, T = 1000, 4000, 0.8
    row = torch.full((V,), -30.0)
    six = [3, 99, 500, 501, 998, 0]
    row[six] = torch.tensor([2.0, 1.0, 0.5, 0.0, -0.5, -1.0])
    kept = W.host_kept(row[None], T, 0, 0.8, 0.0)[0]
    assert kept.nonzero().flatten().tolist() == [3, 99]
    x = row[None, :].repeat(N, 1).cuda()
    state = torch.tensor([7, -1], dtype=torch.int32, device="cuda")
    seed_t = torch.tensor([42], dtype=torch.int64, device="cuda")
    tok = ops.sample_warp(x, T, 0, 0.8, 0.0, seed_t, state).cpu()
    probs = torch.softmax(row.double().masked_fill(~kept, float("-inf")) / T, 0)
    counts = torch.bincount(tok, minlength=V).double()
    for i in (3, 99):
        sd = (N * probs[i] * (1 - probs[i])).sqrt()
        assert abs(counts[i] - N * probs[i]) < 4.5 * sd, (i, float(counts[i]), float(N * probs[i]))
    assert int(counts[~kept].sum()) == 0 and counts.sum() == N
    state2 = torch.tensor([8, -1], dtype=torch.int32, device="cuda")
    assert not torch.equal(ops.sample_warp(x, T, 0, 0.8, 0.0, seed_t, state2).cpu(), tok)
    assert torch.equal(ops.sample_warp(x, T, 0, 0.8, 0.0, seed_t, state).cpu(), tok)


def test_entry_point_refuses_bad_arguments(dev):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    x = torch.zeros(2, 10, device=dev)
    f = torch.empty_like(x)
    for bad in (dict(temperature=0.0), dict(top_p=1.5), dict(min_p=-0.1), dict(min_p=1.5), dict(top_k=-1)):
        a = dict(temperature=1.0, top_k=0, top_p=0.9, min_p=0.0)
        a.update(bad)
        with pytest.raises(MagmaHipError):
            ops.sample_warp(x, a["temperature"], a["top_k"], a["top_p"], a["min_p"], None, None, filtered=f, want_token=False)


# ---- generate() ----
@pytest.fixture(scope="module")
def model(dev):
    from magma_amd.testing import build_reduced_magma
    torch.manual_seed(3)
    m = build_reduced_magma(dev)
    m.eval()
    return m


@pytest.fixture(scope="module")
def emb(model):
    g = torch.Generator().manual_seed(5)
    return model.embed([torch.randn(2, 3, 64, 64, generator=g), torch.randint(0, 1000, (2, 5), generator=g)])


WARP = dict(temperature=0.9, top_k=20, top_p=0.9, min_p=0.05, sampler="transformers")


def _gen(model, emb, n=10, **kw):
    return model.generate(emb, max_steps=n, decode=False, stop_on_eos=False, **kw)


def test_generate_reproducible_and_graph_equals_eager(model, emb):
    a, b, c = _gen(model, emb, seed=123, **WARP), _gen(model, emb, seed=123, **WARP), _gen(model, emb, seed=124, **WARP)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.shape == (2, emb.shape[1] + 10)
    # the same call without the captured graph (eager launches of the same token step)
    eng = model.lm.engine
    mode = ("warp", 0.9, 20, 0.9, 0.05)
    out = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=10, sampling=mode, eos_token=model.eos_token, seed=123)
    toks, cache = [out.next_token.clone()], out.past_key_values
    for _ in range(9):
        _, tk = eng.decode(toks[-1][:, None], cache, use_graph=False, sampling=mode)
        toks.append(tk.clone())
    assert torch.equal(a[:, emb.shape[1]:], torch.stack(toks, 1))
    # the sampler differs from the reference's at the same values and seed somewhere in ten tokens of two rows
    kw = {k: v for k, v in WARP.items() if k not in ("sampler", "min_p")}
    assert not torch.equal(_gen(model, emb, n=24, seed=123, **kw), _gen(model, emb, n=24, seed=123, sampler="transformers", **kw))
    # torch.manual_seed reproduces a run when no seed is passed
    torch.manual_seed(77); d1 = _gen(model, emb, n=6, temperature=0.7, sampler="transformers")
    torch.manual_seed(77); d2 = _gen(model, emb, n=6, temperature=0.7, sampler="transformers")
    assert torch.equal(d1, d2)
    strs = model.generate(emb, max_steps=4, temperature=0.7, top_k=5, top_p=0.9, sampler="transformers", min_p=0.1)
    assert isinstance(strs, list) and len(strs) == 2


def test_generate_degenerate_settings_equal_greedy(model, emb):
    greedy = _gen(model, emb, temperature=0.0)
    assert torch.equal(_gen(model, emb, temperature=0.7, top_p=1e-6, seed=1, sampler="transformers"), greedy)
    assert torch.equal(_gen(model, emb, temperature=1.3, top_p=0.0, min_p=1.0, seed=2, sampler="transformers"), greedy)
    assert torch.equal(_gen(model, emb, temperature=0.7, top_k=1, top_p=0.0, seed=3, sampler="transformers"), greedy)
    assert not torch.equal(_gen(model, emb, temperature=1.3, top_p=0.0, seed=2, sampler="transformers"), greedy)


def test_generate_combines_with_processors_stopping_ragged_and_caches(model, emb):
    S = emb.shape[1]
    plain = _gen(model, emb, seed=11, **WARP)[:, S:]
    # logits processors in front of the selection: a suppressed id never appears
    banned = tuple(dict.fromkeys(plain.flatten().tolist()))[:4]
    got = _gen(model, emb, seed=11, repetition_penalty=1.3, suppress_tokens=banned, **WARP)[:, S:]
    assert not set(got.flatten().tolist()) & set(banned) and not torch.equal(got, plain)
    # per-row stopping: row 0 stops on the two tokens it drew at steps 2 and 3, row 1 (same stream) is what it was
    seq = plain[0, 2:4].tolist()
    first = next(i for i in range(1, 10) if plain[0, i - 1:i + 1].tolist() == seq)
    out, fin = model.generate(emb, max_steps=10, decode=False, stop_on_eos=False, seed=11, stop_sequences=[seq],
                              return_finish=True, **WARP)
    assert fin.reason[0] == "stop" and int(fin.kept[0]) == first + 1
    assert torch.equal(out[0, S:S + first + 1], plain[0, :first + 1]) and bool((out[0, S + first + 1:] == model.eos_token).all())
    if fin.reason[1] == "length":
        assert torch.equal(out[1, S:], plain[1])
    # ragged batch: reproducible, and the degenerate nucleus is the ragged greedy call
    lengths = [S, S - 3]
    r1, r2 = _gen(model, emb, seed=11, lengths=lengths, **WARP), _gen(model, emb, seed=11, lengths=lengths, **WARP)
    assert torch.equal(r1, r2) and torch.equal(r1[0, S:], plain[0])           # row 0 is full length: the row it was
    assert torch.equal(_gen(model, emb, lengths=lengths, temperature=0.7, top_p=1e-6, seed=1, sampler="transformers"),
                       _gen(model, emb, lengths=lengths, temperature=0.0))
    # continued caches: what the existing multi-turn test claims for the reference's sampler -- the sampler that can only
    # pick the top token continues exactly as greedy decoding does -- and a sampled continuation is reproducible
    q = emb[:, :4].contiguous()
    kw = dict(max_steps=5, decode=False, eos_token=-7)
    _, p1 = model.generate(emb, temperature=0.0, return_past_key_values=True, **kw)
    g = model.generate(q, temperature=0.0, past_key_values=p1, **kw)
    _, p2 = model.generate(emb, temperature=1.0, top_p=1e-6, seed=9, sampler="transformers", return_past_key_values=True, **kw)
    s = model.generate(q, temperature=1.0, top_p=0.0, min_p=1.0, seed=9, sampler="transformers", past_key_values=p2, **kw)
    assert torch.equal(g, s)
    conts = []
    for _ in range(2):
        _, p = model.generate(emb, seed=21, return_past_key_values=True, **kw, **WARP)
        conts.append(model.generate(q, seed=22, past_key_values=p, **kw, **WARP))
    assert torch.equal(conts[0], conts[1])


def test_defaults_untouched_and_one_selection_launch(model, emb, monkeypatch):
    from launch_trace import record
    from magma_amd import ops
    eng = model.lm.engine
    kw = dict(temperature=0.7, top_k=0, top_p=0.9, seed=3)
    assert torch.equal(_gen(model, emb, **kw), _gen(model, emb, sampler="reference", **kw))
    calls = []
    real = ops.sample_warp
    monkeypatch.setattr(ops, "sample_warp", lambda *x, **k: (calls.append(1), real(*x, **k))[1])
    orig = eng.decode
    monkeypatch.setattr(eng, "decode", lambda *x, **k: orig(*x, **{**k, "use_graph": False}))
    rec_a, out_a = record(eng, lambda: _gen(model, emb, 5, **kw))
    rec_b, out_b = record(eng, lambda: _gen(model, emb, 5, sampler="reference", min_p=0.0, **kw))
    assert not isinstance(out_a, Exception) and not isinstance(out_b, Exception), (out_a, out_b)
    assert torch.equal(out_a, out_b) and rec_a == rec_b and len(rec_a) > 20
    assert not calls and sum(r["op"] == "sample" for r in rec_a) == 5
    # transformers' sampler: the reference's launches with the one selection launch exchanged, and none more
    rec_w, out_w = record(eng, lambda: _gen(model, emb, 5, sampler="transformers", min_p=0.05, **kw))
    assert not isinstance(out_w, Exception), out_w
    assert len(calls) == 5
    assert [r["op"] for r in rec_w] == [r["op"] for r in rec_a if r["op"] != "sample"]
    at = [i for i, r in enumerate(rec_a) if r["op"] == "sample"]
    assert all(rec_a[i + 1]["op"] == "sample_finish" for i in at)      # ... which sits where `sample` sat: right before the bookkeeping
