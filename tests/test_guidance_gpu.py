"""Classifier-free guidance on the device (DESIGN.md "Classifier-free guidance"): the pair kernel (ops.logits_guidance) against the
float64 host statement (magma_amd.sampling.guide_logits, pinned to transformers by tests/test_guidance_cpu.py) per element within
the bound G derived there, its plausibility cut as an exact set, ops.guidance_follow, and generate(guidance_scale=...) on the
reduced model: the device's tokens followed through a teacher-forced replay of the engine's own eager 2B-row decode, captured
steps against eager ones under every combination, a reused cache, the unguided call afterwards, W4A16, the wide step, and the
number of launches a guided step adds."""
import types
import warnings

import pytest
import torch

from test_beam_search_gpu import _emb, _gapped_logits, _model
from test_guidance_cpu import guidance_bound
from test_logits_processors_gpu import _rows

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
SENT = 1.0e30               # the padding would change every maximum if read


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------- the kernel
def _launch(dev, cond, uncond, scale, min_p, shift=0):
    """One launch with both operands inside buffers of V + 7 columns and R + 2 rows filled with a sentinel (``shift``: the
    unconditional rows start that many columns in, so that the two rows of a pair differ in their 16-byte phase).  Returns the
    guided rows on the host after checking that the unconditional buffer, the padding and the guard rows kept their bits."""
    from magma_amd import ops
    R, V = cond.shape
    big_c = torch.full((R + 2, V + 7), SENT, device=dev)
    big_u = torch.full((R + 2, V + 7), SENT, device=dev)
    big_c[1:R + 1, :V] = cond.to(dev)
    big_u[1:R + 1, shift:shift + V] = uncond.to(dev)
    before_c, before_u = big_c.clone(), big_u.clone()
    ops.logits_guidance(big_c[1:R + 1, :V], big_u[1:R + 1, shift:shift + V], scale, min_p)
    assert torch.equal(_bits(big_u), _bits(before_u))
    keep = torch.ones_like(big_c, dtype=torch.bool)
    keep[1:R + 1, :V] = False
    assert torch.equal(_bits(big_c[keep]), _bits(before_c[keep]))
    return big_c[1:R + 1, :V].cpu()


def _pair(R, V, seed):
    """Gapped rows; row 0 carries a conditional -inf, the last row a +60 outlier (one row carries both when R = 1)."""
    cond, uncond = _gapped_logits(R, V, seed), _gapped_logits(R, V, seed + 1)
    cond[0, 2 % V] = NEG_INF
    cond[R - 1, V - 1] += 60.0
    return cond, uncond


def _compare(got, cond, uncond, scale, min_p, what):
    """-inf exactly where the statement has it (the kept set of the cut included), every other value within G."""
    from magma_amd.sampling import guide_logits
    ref = guide_logits(cond, uncond, scale, min_p)
    inf = torch.isinf(ref)
    assert torch.equal(got == NEG_INF, inf) and not bool(torch.isnan(got).any()), what
    ratio = ((got.double() - ref).abs() / guidance_bound(cond, uncond, scale))[~inf]
    print(f"{what}: max err / G = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0, (what, float(ratio.max()))
    return int(inf.sum())


@pytest.mark.parametrize("V", [7, 64, 1025, 50258])
@pytest.mark.parametrize("R", [1, 3, 17])
def test_kernel_equals_statement(dev, R, V):
    cond, uncond = _pair(R, V, seed=11 * V + R)
    for scale in (0.0, 1.5, 7.5):
        for min_p in (0.0, 0.1):
            for shift in (0, 1):
                got = _launch(dev, cond, uncond, scale, min_p, shift)
                n_inf = _compare(got, cond, uncond, scale, min_p, f"V={V} R={R} s={scale} min_p={min_p} shift={shift}")
                # the conditional -inf stays -inf; the cut removes more (beside the +60 outlier nothing is plausible)
                assert n_inf >= 1 and (n_inf == 1) == (min_p == 0.0)


def test_kernel_cut_threshold_in_fp32(dev):
    """A tie at the bound stays, one ulp below goes, min_p = 1 keeps exactly the maxima: host and device keep the same set."""
    from magma_amd.sampling import guide_logits
    V = 1025
    cond, uncond = _gapped_logits(2, V, 3), _gapped_logits(2, V, 4)
    cond = cond - cond.max(-1, keepdim=True).values - 3.0
    cond[:, 9], cond[0, 700] = 0.0, 0.0
    bound = torch.tensor(0.1, dtype=torch.float64).log().to(torch.float32)
    cond[0, 5], cond[0, 6], cond[1, 1024] = bound, torch.nextafter(bound, torch.tensor(NEG_INF)), bound
    for min_p, kept in ((0.1, [[0, 5], [0, 9], [0, 700], [1, 9], [1, 1024]]), (1.0, [[0, 9], [0, 700], [1, 9]])):
        got = _launch(dev, cond, uncond, 2.0, min_p)
        assert (got > NEG_INF).nonzero().tolist() == kept
        assert torch.equal(got > NEG_INF, guide_logits(cond, uncond, 2.0, min_p) > NEG_INF)


@pytest.mark.parametrize("V", [7, 1025, 50258])
def test_kernel_equal_rows_give_equal_bits_at_every_scale(dev, V):
    """uncond bitwise equal to cond: c - u = 0 and s * 0 is exact, so every scale writes the bits of the log_softmax."""
    from magma_amd.sampling import guide_logits
    cond, _ = _pair(3, V, seed=V)
    cond[0, 2 % V] = 0.25           # (the unconditional rows must be finite)
    outs = [_launch(dev, cond, cond.clone(), scale, 0.0, shift) for scale in (0.0, 1.5, 7.5) for shift in (0, 1)]
    assert all(torch.equal(_bits(o), _bits(outs[0])) for o in outs[1:])
    _compare(outs[0], cond, cond, 1.0, 0.0, f"equal rows V={V}")
    assert torch.equal(guide_logits(cond, cond, 7.5), guide_logits(cond, cond, 0.0))


def test_kernel_refuses_bad_arguments(dev):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    c, u = torch.zeros(2, 9, device=dev), torch.zeros(2, 9, device=dev)
    for scale in (-1.0, float("nan"), float("inf")):
        with pytest.raises(MagmaHipError):
            ops.logits_guidance(c, u, scale)
    with pytest.raises(ValueError):
        ops.logits_guidance(c, u, 2.0, min_p=1.5)
    lib = ops.L.load()
    for rc in (lib.mg_guidance_follow(None, None, 2, 1, 1, None), lib.mg_guidance_follow(c.data_ptr(), None, 0, 1, 1, None),
               lib.mg_guidance_follow(c.data_ptr(), None, 2, 1, 2, None),
               lib.mg_logits_guidance_f32(c.data_ptr(), 8, u.data_ptr(), 9, 2, 9, 1.0, 0.0, None),
               lib.mg_logits_guidance_f32(c.data_ptr(), 9, None, 9, 2, 9, 1.0, 0.0, None),
               lib.mg_logits_guidance_f32(c.data_ptr(), 9, u.data_ptr(), 9, 2, 9, 1.0, 0.5, None)):
        with pytest.raises(MagmaHipError):
            ops.L.check(rc, "refused")
    torch.cuda.synchronize()
    assert float(c.abs().sum()) == 0.0          # nothing was launched


@pytest.mark.parametrize("R", [1, 5, 17])
def test_guidance_follow(dev, R):
    from magma_amd import ops
    g = torch.Generator().manual_seed(R)
    tok = torch.randint(0, 50000, (2 * R + 2,), generator=g)
    pos = torch.randint(1, 300, (2 * R + 2,), generator=g).to(torch.int32)
    for delta in (1, 3):
        t_d, p_d = tok.to(dev), pos.to(dev)
        ops.guidance_follow(t_d[1:2 * R + 1], p_d[1:2 * R + 1], R, delta, pos_stride=1)
        want_t, want_p = tok.clone(), pos.clone()
        want_t[1 + R:1 + 2 * R] = tok[1:1 + R]
        want_p[1 + R:1 + 2 * R] += delta
        assert torch.equal(t_d.cpu(), want_t) and torch.equal(p_d.cpu(), want_p), (R, delta)
    t_d = tok.to(dev)            # no positions (the first token of a loop): the tokens alone
    ops.guidance_follow(t_d[1:2 * R + 1], None, R)
    assert torch.equal(t_d.cpu(), want_t)


# ------------------------------------------------------------------------------------------------------- the reduced model
B, S, S_NEG, N = 3, 7, 3, 8
LENS, NEG_LENS = [7, 4, 5], [3, 2, 3]
SEED = 21                   # at this seed the guided ids differ from the unguided call's (asserted below)


@pytest.fixture(scope="module")
def model(dev):
    return _model(dev)


def _inputs(model, seed=SEED, b=B):
    return _emb(model, b, S, seed), _emb(model, b, S_NEG, seed + 500)


def _gen(model, emb, neg, n=N, lens=LENS, neg_lens=NEG_LENS, **kw):
    kw.setdefault("temperature", 0.0)
    kw.setdefault("guidance_scale", 3.0)
    kw.setdefault("stop_on_eos", False)
    return model.generate(emb, max_steps=n, decode=False, lengths=lens, negative_embeddings=neg, negative_lengths=neg_lens, **kw)


def _both(emb, neg, lens, neg_lens):
    """The 2B ragged rows of a guided call: the prompts, then the negative prompts."""
    b = emb.shape[0]
    both = torch.zeros(2 * b, max(emb.shape[1], neg.shape[1]), emb.shape[2], dtype=emb.dtype, device=emb.device)
    both[:b, :emb.shape[1]], both[b:, :neg.shape[1]] = emb, neg
    return both, torch.tensor(list(lens) + list(neg_lens), dtype=torch.int64)


def _replay(model, emb, neg, tokens, lens=LENS, neg_lens=NEG_LENS):
    """The RAW fp32 logits (2B, V) every step of a guided run over ``tokens`` (B, n) selected from: the prefill over both halves,
    then eager teacher-forced unguided 2B-row decode steps fed the device's tokens -- the kernels of the run, so its logits."""
    eng = model.lm.engine
    both, all_lens = _both(emb, neg, lens, neg_lens)
    o = eng.forward(inputs_embeds=both, use_cache=True, cache_hint=tokens.shape[1], lengths=all_lens)
    c = o.past_key_values
    out = [o.logits[:, -1].float().cpu()]
    for t in range(tokens.shape[1] - 1):
        ids = tokens[:, t].repeat(2).view(-1, 1).to(model.device)
        out.append(eng.decode(ids, c, use_graph=False)[0].float().cpu())
    return out


def _follows(raw, tokens, eos, scale=3.0, min_p=0.0, rules=None):
    """At every step and row the device's token is, on the host statement over the replayed logits, within 2 G_max of the best
    (G_max: the largest G of the row; a repetition penalty p scales a value, and so its error, by at most p)."""
    from magma_amd.sampling import guide_logits, process_logits
    b = tokens.shape[0]
    for t, lg in enumerate(raw):
        host = guide_logits(lg[:b], lg[b:], scale, min_p)
        tol = 2.0 * guidance_bound(lg[:b], lg[b:], scale).max(-1).values
        if rules:
            host = process_logits(host.float(), tokens, t, eos_token=eos, **rules).double()
            tol = tol * max(rules.get("repetition_penalty", 1.0), 1.0) + 2.0 ** -22 * host.max(-1).values.abs()
        chosen = host.gather(1, tokens[:, t:t + 1])[:, 0]
        assert bool((chosen >= host.max(-1).values - tol).all()), (t, chosen, host.max(-1).values, tol)


def _eager(model, monkeypatch, fn):
    """``fn()`` with every token step launched eagerly instead of replayed from its captured graph."""
    eng = model.lm.engine
    orig = eng.decode
    with monkeypatch.context() as m:
        m.setattr(eng, "decode", lambda *x, **k: orig(*x, **{**k, "use_graph": False}))
        return fn()


def test_generate_follows_the_statement(model):
    emb, neg = _inputs(model)
    eos = model.eos_token
    plain = model.generate(emb, max_steps=N, temperature=0.0, decode=False, stop_on_eos=False, lengths=LENS)
    out = _gen(model, emb, neg)
    assert out.shape == plain.shape
    width = torch.arange(out.shape[1])[None, :]
    assert bool((out.cpu()[width < torch.tensor(LENS)[:, None]] == model.image_token).all())      # the unguided call's layout
    assert bool((out.cpu()[width >= torch.tensor(LENS)[:, None] + N] == eos).all())
    toks = _rows(out, S, N, LENS)
    assert not torch.equal(toks, _rows(plain, S, N, LENS)), "the guidance changed no token: pick another SEED"
    raw = _replay(model, emb, neg, toks)
    _follows(raw, toks, eos)
    # a second call on the reused cache (every step replayed) equals the first (first step eager, second captured)
    assert torch.equal(_gen(model, emb, neg), out)
    # the plausibility cut
    cut = _gen(model, emb, neg, guidance_min_p=0.1)
    toks_cut = _rows(cut, S, N, LENS)
    _follows(_replay(model, emb, neg, toks_cut), toks_cut, eos, min_p=0.1)
    # one negative row shared by every sample, lengths given as embed_batch's pair
    one = _gen(model, emb, (neg[:1], torch.tensor([2])), neg_lens=None)
    toks_one = _rows(one, S, N, LENS)
    _follows(_replay(model, emb, neg[:1].expand(B, -1, -1), toks_one, neg_lens=[2] * B), toks_one, eos)


VARIANTS = {"min_p": dict(guidance_min_p=0.1),
            "sampled": dict(sampler="transformers", temperature=0.8, top_k=12, top_p=0.9, min_p=0.02, seed=77),
            "reference sampler": dict(temperature=0.8, top_k=12, top_p=0.9, seed=77),
            "penalty": dict(repetition_penalty=1.3)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_captured_steps_equal_eager_steps(model, monkeypatch, variant):
    emb, neg = _inputs(model)
    kw = VARIANTS[variant]
    out = _gen(model, emb, neg, **kw)
    assert torch.equal(_gen(model, emb, neg, **kw), out)
    assert torch.equal(_eager(model, monkeypatch, lambda: _gen(model, emb, neg, **kw)), out)
    if variant == "penalty":
        toks = _rows(out, S, N, LENS)
        _follows(_replay(model, emb, neg, toks), toks, model.eos_token, rules=kw)


def test_per_row_stopping_and_finish(model, monkeypatch):
    emb, neg = _inputs(model)
    toks = _rows(_gen(model, emb, neg), S, N, LENS)
    eos = model.eos_token
    r = next(b for b in range(B) if eos not in toks[b, :2].tolist())       # a row that generates two tokens before its eos
    kw = dict(stop_sequences=[toks[r, :2].tolist()], return_finish=True, stop_on_eos=True)
    out, fin = _gen(model, emb, neg, **kw)
    assert fin.reason[r] == "stop" and int(fin.kept[r]) == 2
    n = out.shape[1] - S
    got = _rows(out, S, n, LENS)
    for b in range(B):
        k = int(fin.kept[b])
        assert torch.equal(got[b, :k], toks[b, :k]) and bool((got[b, k:] == model.eos_token).all())     # padded once finished
    out2, fin2 = _eager(model, monkeypatch, lambda: _gen(model, emb, neg, **kw))
    assert torch.equal(out2, out) and fin2.reason == fin.reason and torch.equal(fin2.kept, fin.kept)


def test_logprobs_stay_those_of_the_raw_conditional_rows(model, monkeypatch):
    from test_logprobs_gpu import _check_against
    emb, neg = _inputs(model)
    plain = _gen(model, emb, neg)
    for rules in ({}, dict(repetition_penalty=1.3)):
        want = _gen(model, emb, neg, **rules)
        out, lps = _gen(model, emb, neg, return_logprobs=True, top_logprobs=3, **rules)
        assert torch.equal(out, want)                                   # the flags change no id
        toks = _rows(out, S, N, LENS)
        assert torch.equal(lps.tokens, toks)
        raw = [lg[:B] for lg in _replay(model, emb, neg, toks)]
        _check_against(lps, raw, model.lm.engine.V, f"guided {sorted(rules)}")
        out2, lps2 = _eager(model, monkeypatch, lambda: _gen(model, emb, neg, return_logprobs=True, top_logprobs=3, **rules))
        assert torch.equal(out2, out) and all(torch.equal(a, b) for a, b in zip(lps2, lps))
    assert torch.equal(_gen(model, emb, neg), plain)


def test_constraint_and_choose(model, monkeypatch):
    from magma_amd.sampling import TokenTrie
    from test_constrained_gpu import _choices, _listed
    emb, neg = _inputs(model)
    eos, V = model.eos_token, model.lm.engine.V
    plain = _rows(_gen(model, emb, neg), S, N, LENS)
    rows = [_choices(plain, eos, V, seed=b, count=4 + b) for b in range(B)]
    tries = [TokenTrie(r) for r in rows]
    out = _gen(model, emb, neg, constraint=rows)
    got = _rows(out, S, N, LENS)
    assert all(_listed(r, t, eos) for r, t in zip(got, tries)), got
    assert torch.equal(_eager(model, monkeypatch, lambda: _gen(model, emb, neg, constraint=rows)), out)
    index, lps = model.choose(emb, rows, lengths=LENS, guidance_scale=3.0, negative_embeddings=neg, negative_lengths=NEG_LENS)
    assert all(0 <= int(i) < len(r) for i, r in zip(index, rows))
    for b in range(B):
        seq = rows[b][int(index[b])]
        assert got[b, :len(seq)].tolist() == seq and lps.count[b] == len(seq) + 1


def test_unguided_call_afterwards_is_the_fresh_engines(dev, model):
    emb, neg = _inputs(model)
    _gen(model, emb, neg)
    _gen(model, emb, neg, return_logprobs=True, constraint=[[5, 6], [7]], repetition_penalty=1.2)
    fresh = _model(dev)
    both, all_lens = _both(emb, neg, LENS, NEG_LENS)        # six unguided rows: the pooled cache of the guided call
    for e, l in ((emb, LENS), (both, all_lens.tolist())):
        for kw in (dict(temperature=0.0), dict(temperature=0.8, top_k=12, seed=5), dict(temperature=0.0, repetition_penalty=1.3,
                                                                                       constraint=[[5, 6], [7]], return_logprobs=True)):
            a = model.generate(e, max_steps=N, decode=False, stop_on_eos=False, lengths=l, **kw)
            b = fresh.generate(e, max_steps=N, decode=False, stop_on_eos=False, lengths=l, **kw)
            a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
            assert torch.equal(a[0], b[0])
            assert len(a) == 1 or all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    # and the guided call on the engine that served them equals the guided call on the fresh one
    assert torch.equal(_gen(model, emb, neg), _gen(fresh, emb, neg))


def test_wide_step(model):
    """2B = 18 rows: the eager tile-GEMM step."""
    emb, neg = _inputs(model, seed=SEED + 1, b=9)
    lens, neg_lens = [7, 4, 5] * 3, [3, 2, 3] * 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (the engine says once that this step is the slow one)
        out = _gen(model, emb, neg, n=4, lens=lens, neg_lens=neg_lens)
    toks = _rows(out, S, 4, lens)
    _follows(_replay(model, emb, neg, toks, lens, neg_lens), toks, model.eos_token)


@pytest.mark.parametrize("switch", ["MAGMA_DECODE_W4", "MAGMA_DECODE_W8"])
def test_quantised_decode(dev, monkeypatch, switch):
    """W4A16 / W8A16 at 2B = 6 rows: the quantised step runs and its tokens follow the statement on its own replayed logits."""
    from test_w4a16_gpu import _model as _w4_model
    if switch.endswith("W4"):
        model = _w4_model(dev, monkeypatch)
    else:       # W8A16 takes adapter projections with K % 1024 == 0: the one-block d = 4096 model of the constrained tests
        model = _model(dev, monkeypatch, w8=True, n_layer=1, n_head=16, d_ff=4096)
    emb, neg = _inputs(model)
    out = _gen(model, emb, neg)
    toks = _rows(out, S, N, LENS)
    cache = next(iter(model.lm.engine._cache_pool.values()))
    st = cache.decode_state
    assert (st.w4, st.w8) == (switch.endswith("W4"), switch.endswith("W8")) and st.refusal is None and cache.B == 2 * B
    _follows(_replay(model, emb, neg, toks), toks, model.eos_token)
    assert torch.equal(_gen(model, emb, neg), out)


def test_refusals_on_the_engine(model):
    emb, neg = _inputs(model)
    eng = model.lm.engine
    both, all_lens = _both(emb, neg, LENS, NEG_LENS)
    with pytest.raises(NotImplementedError):
        eng.forward(inputs_embeds=both, use_cache=True, lengths=all_lens, eos_token=model.eos_token, guidance=(3.0, 0.0),
                    beam=(2, 1.0, False, 4))
    with pytest.raises(ValueError):         # one shared position: not a guided batch
        eng.forward(inputs_embeds=both, use_cache=True, eos_token=model.eos_token, guidance=(3.0, 0.0))
    with pytest.raises(ValueError):
        eng.forward(inputs_embeds=both[:5], use_cache=True, lengths=all_lens[:5], eos_token=model.eos_token, guidance=(3.0, 0.0))
    with pytest.raises(ValueError):
        eng.guidance_mode((-1.0, 0.0))
    for kw in (dict(num_beams=2), dict(return_past_key_values=True)):
        with pytest.raises(NotImplementedError):
            _gen(model, emb, neg, **kw)


# ----------------------------------------------------------------------------------------------------------- launch count
_HOST_HELPERS = {"ceil_to", "zero_page", "stop_table", "trie_path", "check"}


def _step_ops(model, monkeypatch, guided, **kw):
    """The names of the ops calls of ONE eager token step over the 2B rows, guided or not."""
    from magma_amd import ops
    eng = model.lm.engine
    emb, neg = _inputs(model)
    both, all_lens = _both(emb, neg, LENS, NEG_LENS)
    gd = dict(guidance=(3.0, 0.1)) if guided else {}
    o = eng.forward(inputs_embeds=both, use_cache=True, cache_hint=4, lengths=all_lens, eos_token=model.eos_token, **gd, **kw)
    calls = []
    with monkeypatch.context() as m:
        for name, fn in list(vars(ops).items()):
            if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_") \
                    and name not in _HOST_HELPERS:
                m.setattr(ops, name, lambda *a, _f=fn, _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
        eng.decode(None, o.past_key_values, use_graph=False, **gd, **kw)
    return calls


@pytest.mark.parametrize("case", ["plain", "processors", "sampled", "stop"])
def test_a_guided_step_adds_two_launches(model, monkeypatch, case):
    extra = {"plain": dict(), "processors": dict(processors=dict(repetition_penalty=1.3, suppress_tokens=(3,))),
             "sampled": dict(sampling=(0.8, 12, 0.9)),
             "stop": dict(stop=dict(eos_ids=(model.eos_token, 2), stop_seqs=((4, 5),)))}[case]
    plain = _step_ops(model, monkeypatch, False, **extra)
    guided = _step_ops(model, monkeypatch, True, **extra)
    assert len(guided) == len(plain) + 2 and len(plain) > 5
    rest = list(guided)
    rest.remove("logits_guidance")
    rest.remove("guidance_follow")
    assert rest == plain and guided[-1] == "guidance_follow"
    sel = "sample" if "sampling" in extra else "argmax"
    first = "logits_process" if "processors" in extra else sel
    assert guided[guided.index("logits_guidance") + 1] == first         # in front of the processors and the selection


# ------------------------------------------------------------------------------------------------- the text-only prompt
def test_embed_batch_drop_images(model):
    g = torch.Generator().manual_seed(3)
    ids = [torch.randint(0, 1000, (1, n), generator=g) for n in (4, 2, 3)]
    img = torch.randn(1, 3, 64, 64, generator=g)
    batch = [[img, ids[0]], [ids[1], img, ids[2]], [ids[2]]]
    emb, lens = model.embed_batch(batch, drop_images=True)
    want, want_lens = model.embed_batch([[ids[0]], [ids[1], ids[2]], [ids[2]]])
    assert torch.equal(lens, want_lens) and lens.tolist() == [4, 5, 3] and torch.equal(emb, want)
    assert len(batch[0]) == 2 and len(batch[1]) == 3 and batch[0][0] is img          # the caller's lists are left as they are
    with pytest.raises(ValueError):
        model.embed_batch([[ids[0]], [img]], drop_images=True)
