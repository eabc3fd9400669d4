"""Token log-probabilities on the device (DESIGN.md "Token log-probabilities"): the kernel (ops.token_logprobs) against the
float64 host statement (magma_amd.sampling.token_logprobs, tests/test_logprobs_cpu.py) and against the beam step's selection
kernel whose device code it shares; generate(return_logprobs=True, top_logprobs=...) on the reduced model against the statement
applied to the RAW logits of a teacher-forced replay through the engine's own eager decode; Magma.score against the loss
forward's target logits; and generate against score on the same tokens (GEMV decode against GEMM prefill).

The value bound, per element, against the float64 statement:  E = 2^-22 max(1, |lp|) + (ceil(V / 1024) + 16) 2^-24.
The first term covers the two roundings at the magnitude of the result ((x - m), then - lse), the second the worst-case fp32
sum of the 1024 strided partials of ceil(V / 1024) terms each plus the 16-wave tree, expf and logf (the sum lies in [1, V], so
its relative error is the absolute error of its logarithm)."""
import math

import pytest
import torch

from test_beam_search_gpu import _emb, _gapped_logits, _model
from test_logits_processors_gpu import _rows

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENT = -77
NEG_INF = float("-inf")


def _bound(lp, V):
    return 2.0 ** -22 * lp.abs().clamp(min=1.0) + (math.ceil(V / 1024) + 16) * 2.0 ** -24


def _within(got, ref, V, what=""):
    """got fp32, ref float64; -inf must match -inf."""
    got = got.double()
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and bool((got[inf] == ref[inf]).all()), what
    err, E = (got - ref)[~inf].abs(), _bound(ref[~inf], V)
    worst = float((err / E).max()) if err.numel() else 0.0
    print(f"{what}: max |err| {float(err.max()) if err.numel() else 0.0:.3e}, max err / E {worst:.3f}")
    assert worst <= 1.0, (what, worst)


# ------------------------------------------------------------------------------------------------------------- the kernel
def _launch(dev, x, tok, n_top, state=None, cols=3):
    """One launch with every operand inside a larger sentinel-filled buffer.  Returns (lp (R, cols), top_id (R, cols, n_top),
    top_lp, the column written or None) as host copies, after checking that nothing outside the windows -- and no other column
    inside them -- was touched."""
    from magma_amd import ops
    R, V = x.shape
    big_x = torch.full((R, V + 7), 1.0e30, device=dev)          # the padding columns would change every maximum if read
    big_x[:, :V] = x.to(dev)
    big_lp = torch.full((R + 2, cols + 5), float(SENT), device=dev)
    big_id = torch.full((R + 2, cols, n_top), SENT, dtype=torch.int32, device=dev)
    big_tl = torch.full((R + 2, cols, n_top), float(SENT), device=dev)
    big_tok = torch.full((R + 2,), 3, dtype=torch.int64, device=dev)
    big_tok[1:R + 1] = tok.to(dev)
    lp, tid, tl = big_lp[1:R + 1, 2:2 + cols], big_id[1:R + 1], big_tl[1:R + 1]
    st = None if state is None else torch.tensor([state, -1], dtype=torch.int32, device=dev)
    ops.token_logprobs(big_x[:, :V], big_tok[1:R + 1], lp, tid if n_top else None, tl if n_top else None, state=st)
    c = 0 if state is None else state
    c = c if 0 <= c < cols else None
    big_lp, big_id, big_tl = big_lp.cpu(), big_id.cpu(), big_tl.cpu()
    keep = torch.ones_like(big_lp, dtype=torch.bool)
    keep3 = torch.ones(R + 2, cols, dtype=torch.bool)
    if c is not None:
        keep[1:R + 1, 2 + c] = False
        keep3[1:R + 1, c] = False
    assert bool((big_lp[keep] == SENT).all()) and bool((big_id[keep3] == SENT).all()) and bool((big_tl[keep3] == SENT).all())
    assert st is None or st.tolist() == [state, -1]
    return big_lp[1:R + 1, 2:2 + cols], big_id[1:R + 1], big_tl[1:R + 1], c


def _tops(V):
    return [n for n in (0, 1, 5, 20) if n <= V] + ([7] if V == 7 else [])


SHAPES = [(V, R) for V in (7, 64, 1025, 50258) for R in (1, 5, 17)]


@pytest.mark.parametrize("V,R", SHAPES)
def test_kernel_equals_statement_on_gapped_logits(dev, V, R):
    """(a): ids equal the float64 top-k exactly, values and the lp of a random token per row are within E."""
    from magma_amd.sampling import token_logprobs
    x = _gapped_logits(R, V, seed=3 * V + R)
    tok = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(V + R))
    for n_top in _tops(V):
        lp, tid, tl, c = _launch(dev, x, tok, n_top)
        r_lp, r_id, r_tl = token_logprobs(x, tok, n_top)
        assert c == 0 and torch.equal(tid[:, 0].long(), r_id), (n_top, tid[:, 0], r_id)
        assert torch.equal(r_id, torch.topk(x.double(), n_top, dim=-1)[1])
        _within(lp[:, 0], r_lp, V, f"lp V={V} R={R} n_top={n_top}")
        _within(tl[:, 0], r_tl, V, f"top_lp V={V} R={R} n_top={n_top}")


@pytest.mark.parametrize("V,R", SHAPES)
def test_kernel_has_the_bits_of_the_beam_selection(dev, V, R):
    """(b): the lists with n_top = K2 equal ops.beam_topk(run = 0) by value, exactly: one device body, one arithmetic."""
    from magma_amd import ops
    x = _gapped_logits(R, V, seed=5 * V + R)
    xd = torch.zeros(R, V + 7, device=dev)
    xd[:, :V] = x.to(dev)
    tok = torch.zeros(R, dtype=torch.int64)
    for K2 in [k for k in (2, 8, 20) if k <= V]:
        cs = torch.zeros(R, K2, device=dev)
        ct = torch.zeros(R, K2, dtype=torch.int32, device=dev)
        ops.beam_topk(xd[:, :V], torch.zeros(R, device=dev), cs, ct)
        lp, tid, tl, _ = _launch(dev, x, tok, K2)
        assert torch.equal(tid[:, 0], ct.cpu()) and bool((tl[:, 0] == cs.cpu()).all()), K2
        # and the token's own value is the list's value where the token is in the list
        lp0, _, tl0, _ = _launch(dev, x, ct[:, 1].cpu().long(), K2)
        assert bool((lp0[:, 0] == tl0[:, 0, 1]).all())


@pytest.mark.parametrize("V,R", SHAPES)
def test_kernel_ties(dev, V, R):
    """(c): the maximum duplicated, and 30 copies (V = 7: 4) of the n-th value: ids equal the stable sort, entry 0 is ops.argmax."""
    from magma_amd import ops
    from magma_amd.sampling import token_logprobs
    g = torch.Generator().manual_seed(7 * V + R)
    copies = min(30, V - 3)
    for n_top in [n for n in _tops(V) if n >= 1]:
        x = _gapped_logits(R, V, seed=11 * V + R + n_top)
        for r in range(R):
            order = torch.sort(x[r], descending=True)[1]
            x[r, int(torch.randint(0, V, (1,), generator=g))] = x[r, order[0]]                  # a second maximum (or the same id)
            nth = torch.sort(x[r], descending=True)[0][n_top - 1]
            low = torch.sort(x[r], descending=True)[1][-copies:]                                # the smallest entries become ties
            x[r, low[torch.randperm(copies, generator=g)]] = nth
        tok = torch.randint(0, V, (R,), generator=g)
        lp, tid, tl, _ = _launch(dev, x, tok, n_top)
        r_lp, r_id, r_tl = token_logprobs(x, tok, n_top)
        assert torch.equal(tid[:, 0].long(), r_id), (n_top, tid[:, 0], r_id)
        assert torch.equal(tid[:, 0, 0].long(), ops.argmax(x.to(dev)).cpu())
        _within(lp[:, 0], r_lp, V, f"ties lp V={V} n_top={n_top}")
        _within(tl[:, 0], r_tl, V, f"ties top_lp V={V} n_top={n_top}")


@pytest.mark.parametrize("V,R", [(7, 5), (1025, 17), (50258, 1)])
def test_kernel_column_guard_and_tokens_outside(dev, V, R):
    """(d) state[0] = cols - 1 writes the last column, cols and cols + 3 write nothing; (e) token -1 and V give -inf, lists intact."""
    from magma_amd.sampling import token_logprobs
    x = _gapped_logits(R, V, seed=V + 13 * R)
    tok = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(R))
    cols, n_top = 3, min(5, V)
    r_lp, r_id, r_tl = token_logprobs(x, tok, n_top)
    for state in (0, cols - 1, cols, cols + 3, -1):
        lp, tid, tl, c = _launch(dev, x, tok, n_top, state=state, cols=cols)       # (_launch checks every other column)
        assert c == (state if 0 <= state < cols else None)
        if c is not None:
            assert torch.equal(tid[:, c].long(), r_id)
            _within(lp[:, c], r_lp, V, f"column {c}")
    for bad in (-1, V, V + 1000, -2 ** 40):
        t2 = tok.clone()
        t2[0] = bad
        lp, tid, tl, _ = _launch(dev, x, t2, n_top)
        assert float(lp[0, 0]) == NEG_INF and torch.equal(tid[:, 0].long(), r_id)
        _within(tl[:, 0], r_tl, V, "lists beside a token outside")
        _within(lp[1:, 0], r_lp[1:], V, "the other rows")


def test_kernel_refuses_bad_n_top(dev):
    """(f): n_top = 21 and n_top > V are errors, and nothing is launched (every buffer keeps its sentinel)."""
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    for V, n_top in ((64, 21), (7, 8), (7, 20)):
        x = torch.zeros(2, V, device=dev)
        lp = torch.full((2, 1), float(SENT), device=dev)
        tid = torch.full((2, 1, n_top), SENT, dtype=torch.int32, device=dev)
        tl = torch.full((2, 1, n_top), float(SENT), device=dev)
        with pytest.raises(MagmaHipError):
            ops.token_logprobs(x, torch.zeros(2, dtype=torch.int64, device=dev), lp, tid, tl)
        torch.cuda.synchronize()
        assert bool((lp == SENT).all()) and bool((tid == SENT).all()) and bool((tl == SENT).all())


# ------------------------------------------------------------------------------------------------------------- the engine
N, LENS = 6, (5, 9, 2)


@pytest.fixture(scope="module")
def oracle(dev):
    """(reduced model carrying the CPU oracle's seeded weights, oracle config, the oracle's LM parameters) -- as the fixture of
    tests/test_continue_generate_gpu.py: adapters scaled up so that rows differ."""
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


def _prompts(model, lens=LENS, seed=31):
    g = torch.Generator().manual_seed(seed)
    d = model.lm.config.hidden_size
    return [(torch.randn(n, d, generator=g) * 0.5).to(BF16).to(model.device) for n in lens]


def _replay(model, prompts, tokens, past=None):
    """The RAW fp32 logits every step of a run over ``tokens`` (B, n) selected from: prefill (or the rows appended to ``past``),
    then eager teacher-forced decode steps without processors -- the kernels of the run, so its logits.  [n] x (B, V) on the host."""
    from magma_amd.sampling import pad_ragged
    eng = model.lm.engine
    emb, lens = (prompts, None) if torch.is_tensor(prompts) else pad_ragged(prompts)         # a tensor: one position for the batch
    o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=tokens.shape[1], past_key_values=past, lengths=lens)
    c = o.past_key_values
    out = [o.logits[:, -1].float().cpu()]
    for t in range(tokens.shape[1] - 1):
        out.append(eng.decode(tokens[:, t:t + 1].to(model.device), c, use_graph=False)[0].float().cpu())
    return out


def _check_against(lps, raw, V, what, count=None):
    """``lps`` equals the statement on the per-step raw logits: ids exact, values within E; masked past ``count``."""
    from magma_amd.sampling import token_logprobs
    B, n = lps.tokens.shape
    k = lps.top_ids.shape[2]
    count = [n] * B if count is None else [int(c) for c in count]
    assert lps.count.tolist() == count and lps.logprobs.shape == (B, n) and lps.top_logprobs.shape == (B, n, k)
    for t in range(n):
        r_lp, r_id, r_tl = token_logprobs(raw[t], lps.tokens[:, t], k)
        live = torch.tensor([t < c for c in count])
        assert torch.equal(lps.top_ids[live, t], r_id[live]), (what, t)
        if bool(live.any()):
            _within(lps.logprobs[live, t], r_lp[live], V, f"{what} step {t} lp")
            _within(lps.top_logprobs[live, t], r_tl[live], V, f"{what} step {t} top")
        assert bool((lps.logprobs[~live, t] == 0.0).all()) and bool((lps.top_ids[~live, t] == -1).all())
        assert bool((lps.top_logprobs[~live, t] == NEG_INF).all())


MODES = {"greedy": dict(temperature=0.0), "sampled": dict(temperature=0.8, top_k=12, top_p=0.9, seed=77),
         "warp": dict(temperature=0.8, top_k=12, top_p=0.9, min_p=0.02, seed=77, sampler="transformers")}


def _gen(model, prompts, n=N, **kw):
    return model.generate(prompts, max_steps=n, decode=False, stop_on_eos=False, **kw)


@pytest.mark.parametrize("mode", list(MODES))
def test_generate_equals_statement_on_replayed_logits(model, monkeypatch, mode):
    kw = MODES[mode]
    prompts = _prompts(model)
    plain = _gen(model, prompts, **kw)
    out, lps = _gen(model, prompts, return_logprobs=True, top_logprobs=3, **kw)
    assert torch.equal(out, plain)                          # unchanged behaviour: the flags change no id
    toks = _rows(out, 0, N, LENS)
    assert torch.equal(lps.tokens, toks)
    _check_against(lps, _replay(model, prompts, toks), 1056, mode)
    if mode == "greedy":
        assert torch.equal(lps.top_ids[:, :, 0], toks) and torch.equal(lps.top_logprobs[:, :, 0], lps.logprobs)
    # no alternatives: the same log-probabilities, empty lists; a second call replays the captured step
    _, lp0 = _gen(model, prompts, return_logprobs=True, **kw)
    assert torch.equal(lp0.logprobs, lps.logprobs) and lp0.top_ids.shape == (3, N, 0)
    out2, lps2 = _gen(model, prompts, return_logprobs=True, top_logprobs=3, **kw)
    assert torch.equal(out2, out) and all(torch.equal(a, b) for a, b in zip(lps2, lps))
    # the captured step equals the eager step
    eng = model.lm.engine
    orig = eng.decode
    monkeypatch.setattr(eng, "decode", lambda *x, **k: orig(*x, **{**k, "use_graph": False}))
    out3, lps3 = _gen(model, prompts, return_logprobs=True, top_logprobs=3, **kw)
    monkeypatch.undo()
    assert torch.equal(out3, out) and all(torch.equal(a, b) for a, b in zip(lps3, lps))


def test_processors_select_from_a_copy_the_numbers_stay_raw(dev):
    """With logits processors on, the tokens are those of the call without log-probabilities and the numbers are the statement on
    the replayed RAW logits -- this fails if the launch reads the processed rows.  On the model of tests/test_beam_search_gpu.py,
    whose greedy rows repeat eos from the first step on: both rules bite."""
    model = _model(dev)
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    prompts = _prompts(model, seed=32)
    n = 8
    plain = _gen(model, prompts, n, temperature=0.0, **rules)
    assert not torch.equal(plain, _gen(model, prompts, n, temperature=0.0)), "the rules changed no token"
    out, lps = _gen(model, prompts, n, temperature=0.0, top_logprobs=3, **rules)
    assert torch.equal(out, plain)
    toks = _rows(out, 0, n, LENS)
    _check_against(lps, _replay(model, prompts, toks), 1056, "processors")
    assert not torch.equal(lps.top_ids[:, :, 0], toks)      # some selected token is not the raw distribution's first
    # decode() hands back the processed rows in that case, as without log-probabilities
    eng = model.lm.engine
    from magma_amd.sampling import pad_ragged
    emb, lens = pad_ragged(prompts)
    res = []
    for lp_mode in (None, 3):
        o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=4, lengths=lens, eos_token=model.eos_token, processors=rules,
                        logprobs=lp_mode)
        res.append(eng.decode(None, o.past_key_values, use_graph=False, processors=rules, logprobs=lp_mode)[0].float().cpu())
    assert torch.equal(res[0], res[1])


def test_per_row_stopping_masks_and_unchanged_ids(model, monkeypatch):
    prompts = _prompts(model, seed=33)
    n = 10
    rows = _rows(_gen(model, prompts, n, temperature=0.0), 0, n, LENS).tolist()
    eos_ids = [rows[0][2], rows[1][6]]
    kw = dict(max_steps=n, temperature=0.0, decode=False, eos_token=eos_ids, return_finish=True)
    ref, fin0 = model.generate(prompts, **kw)
    out, fin, lps = model.generate(prompts, top_logprobs=2, **kw)
    assert torch.equal(out, ref) and torch.equal(fin.kept, fin0.kept) and torch.equal(lps.count, fin.kept)
    width = out.shape[1] - max(LENS)
    assert len(set(fin.kept.tolist())) > 1 and int(fin.kept.min()) < width, fin
    toks = _rows(out, 0, width, LENS)
    _check_against(lps, _replay(model, prompts, toks), 1056, "per-row", count=fin.kept)
    eng = model.lm.engine
    orig = eng.decode
    monkeypatch.setattr(eng, "decode", lambda *x, **k: orig(*x, **{**k, "use_graph": False}))
    out_e, _, lps_e = model.generate(prompts, top_logprobs=2, **kw)
    monkeypatch.undo()
    assert torch.equal(out_e, out) and all(torch.equal(a, b) for a, b in zip(lps_e, lps))


def test_pooled_cache_and_continued_conversation(dev, model):
    """A call on the pooled cache equals the call on a fresh model; a continued conversation reports its own tokens only."""
    from magma_amd.testing import build_reduced_magma
    prompts = _prompts(model, seed=34)
    _gen(model, prompts, N, temperature=0.0, top_logprobs=5)                      # the pool's cache has served other calls
    _gen(model, prompts, N + 3, temperature=0.7, seed=5, return_logprobs=True)
    out, lps = _gen(model, prompts, N, temperature=0.0, top_logprobs=3)
    fresh = build_reduced_magma(dev)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    out_f, lps_f = _gen(fresh, prompts, N, temperature=0.0, top_logprobs=3)
    assert torch.equal(out, out_f) and all(torch.equal(a, b) for a, b in zip(lps, lps_f))
    # second turn on the returned cache: n2 columns, equal to the statement on the continued replay
    out1, past, lps1 = model.generate(prompts, max_steps=N, temperature=0.0, decode=False, stop_on_eos=False,
                                      return_past_key_values=True, top_logprobs=2)
    q, n2 = _prompts(model, (3, 1, 4), seed=35), 4
    replay_past = model.generate(prompts, max_steps=N, temperature=0.0, decode=False, stop_on_eos=False,
                                 return_past_key_values=True)[1]
    out2, lps2 = model.generate(q, max_steps=n2, temperature=0.0, decode=False, stop_on_eos=False, past_key_values=past,
                                top_logprobs=2)
    toks2 = _rows(out2, 0, n2, (3, 1, 4))
    assert lps2.tokens.shape == (3, n2) and torch.equal(lps2.tokens, toks2) and lps1.tokens.shape == (3, N)
    _check_against(lps2, _replay(model, q, toks2, past=replay_past), 1056, "second turn")


def test_wide_batch_runs_the_eager_step(model):
    lens = [3 + (b * 5) % 7 for b in range(17)]
    prompts = _prompts(model, lens, seed=36)
    out, lps = _gen(model, prompts, 4, temperature=0.0, top_logprobs=4)
    toks = _rows(out, 0, 4, lens)
    _check_against(lps, _replay(model, prompts, toks), 1056, "B = 17")


@pytest.mark.parametrize("switch", ["MAGMA_DECODE_W8", "MAGMA_DECODE_W4"])
def test_quantised_decode(dev, monkeypatch, switch):
    from test_w4a16_gpu import _model as q_model
    model = q_model(dev, monkeypatch, switch=switch, **({"mlp_factor": 1} if switch == "MAGMA_DECODE_W8" else {}))      # W8A16: K % 1024
    prompts = _prompts(model, seed=37)
    plain = _gen(model, prompts, 5, temperature=0.0)
    out, lps = _gen(model, prompts, 5, temperature=0.0, top_logprobs=3)
    assert torch.equal(out, plain)
    toks = _rows(out, 0, 5, LENS)
    _check_against(lps, _replay(model, prompts, toks), 1056, switch)


def test_full_width_vocabulary(dev):
    """d = 4096, V = 50 258, one block: the full-width launch inside the captured step."""
    model = _model(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=128)
    emb = _emb(model, 2, 5, seed=4)
    kw = dict(temperature=0.9, top_k=40, seed=3)
    out, lps = model.generate(emb, max_steps=6, decode=False, stop_on_eos=False, top_logprobs=20, **kw)
    assert torch.equal(out, model.generate(emb, max_steps=6, decode=False, stop_on_eos=False, **kw))
    _check_against(lps, _replay(model, emb, out[:, 5:].cpu()), 50258, "V = 50258")


def test_errors_before_any_launch(model, monkeypatch):
    from magma_amd import ops
    prompts = _prompts(model)
    for name in ("token_logprobs", "argmax", "gemm", "gemm_skinny", "embedding"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a launch was enqueued"))
    for bad in (dict(top_logprobs=21), dict(top_logprobs=-1), dict(top_logprobs=1057), dict(top_logprobs=2.5)):
        with pytest.raises(ValueError):
            model.generate(prompts, max_steps=3, **bad)
    for beam in (dict(num_beams=2), dict(return_scores=True)):
        with pytest.raises(NotImplementedError):
            model.generate(prompts, max_steps=3, return_logprobs=True, **beam)
    with pytest.raises(NotImplementedError):
        model.lm(inputs_embeds=prompts[0][None], use_cache=True, eos_token=model.eos_token, beam=(2, 1.0, False, 4), logprobs=2)


# ------------------------------------------------------------------------------------------------------------------ score
T_LENS = (4, 1, 7)


def _targets(seed=41):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 1056, (n,), generator=g).tolist() for n in T_LENS]


def _loss_forward(model, prompts, targets):
    """forward(labels=...) over [prompt_b ; wte(targets_b)], right-padded: row b's labels are -100 except at its targets."""
    wte = model.lm.engine.wte
    d = wte.shape[1]
    S = max(p.shape[0] + len(t) for p, t in zip(prompts, targets))
    emb = torch.zeros(len(prompts), S, d, dtype=BF16, device=model.device)
    labels = torch.full((len(prompts), S), -100, dtype=torch.int64)
    for b, (p, t) in enumerate(zip(prompts, targets)):
        L = p.shape[0]
        emb[b, :L] = p
        emb[b, L:L + len(t)] = wte[torch.tensor(t, device=model.device)]
        labels[b, L:L + len(t)] = torch.tensor(t)
    return emb, labels, model.lm(inputs_embeds=emb, labels=labels)


def test_score_equals_statement_on_target_logits_and_the_loss(model):
    from magma_amd import ops
    from magma_amd.sampling import token_logprobs
    prompts, targets = _prompts(model, seed=42), _targets()
    res = model.score(prompts, targets, top_logprobs=4)
    assert res.count.tolist() == list(T_LENS) and res.tokens.shape == (3, 7) and res.top_ids.shape == (3, 7, 4)
    emb, labels, o = _loss_forward(model, prompts, targets)
    flat = torch.tensor([t for row in targets for t in row])
    r_lp, r_id, r_tl = token_logprobs(o.target_logits.float().cpu(), flat, 4)
    at = torch.arange(7)[None, :] < res.count[:, None]
    assert torch.equal(res.tokens[at], flat) and bool((res.tokens[~at] == -100).all())
    assert torch.equal(res.top_ids[at], r_id)
    _within(res.logprobs[at], r_lp, 1056, "score lp")
    _within(res.top_logprobs[at], r_tl, 1056, "score top")
    assert bool((res.logprobs[~at] == 0).all()) and bool((res.top_ids[~at] == -1).all()) and bool((res.top_logprobs[~at] == NEG_INF).all())
    # the mean negative log-probability is the forward's loss (each of the 12 terms within E, so the mean within 2 E: the loss
    # kernel's own rounding is the second E)
    nll = -float(res.logprobs.double().sum() / res.count.sum())
    E = float(_bound(r_lp, 1056).max())
    print(f"nll {nll:.7f} loss {float(o.loss):.7f} diff {abs(nll - float(o.loss)):.3e} 2E {2 * E:.3e}")
    assert abs(nll - float(o.loss)) <= 2 * E
    # the refactored forward: its loss and target logits are the bits of the code path as it was -- rows selected by hand, ln_f,
    # the fp32 head GEMM, ops.cross_entropy
    eng = model.lm.engine
    x, _ = eng._blocks_prefill(emb, None)
    B, S = labels.shape
    tgt = labels[:, 1:].reshape(-1).to(model.device)
    rows = (torch.arange(B, device=model.device)[:, None] * S + torch.arange(S - 1, device=model.device)[None, :]).reshape(-1)
    keep = (tgt != -100).nonzero().squeeze(1)
    xl = ops.layernorm(x.index_select(0, rows[keep]), eng.lnf_g, eng.lnf_b, eng.eps)
    old = torch.empty(xl.shape[0], eng.Vp, dtype=torch.float32, device=model.device)
    ops.gemm(xl, eng.head, out=old)
    old_loss, _ = ops.cross_entropy(old[:, : eng.V], tgt[keep].contiguous())
    assert torch.equal(o.target_logits, old[:, : eng.V]) and torch.equal(o.loss, old_loss) and torch.equal(o.target_rows, rows[keep])
    # the three forms of the prompt and the two forms of the targets give the same result
    from magma_amd.sampling import pad_ragged
    padded = torch.full((3, 9), -100, dtype=torch.int64)
    for b, t in enumerate(targets):
        padded[b, : len(t)] = torch.tensor(t)
    emb_p, lens = pad_ragged(prompts)
    for form in (model.score((emb_p, lens), padded, top_logprobs=4), model.score(emb_p, targets, lengths=lens, top_logprobs=4)):
        assert torch.equal(form.logprobs[:, :7], res.logprobs) and torch.equal(form.top_ids[:, :7], res.top_ids)
    assert torch.equal(model.score(prompts, targets).logprobs, res.logprobs)


def test_score_refusals(model):
    prompts = _prompts(model, seed=43)
    ok = _targets()
    for bad in ([[1, 2], [], [3]], [[1, 2], [1056], [3]], [[1, 2], [-5], [3]], [[1], [2]],
                torch.tensor([[1, -100, 2], [1, 2, 3], [1, 2, -100]]), torch.tensor([[1.0], [2.0], [3.0]])):
        with pytest.raises(ValueError):
            model.score(prompts, bad)
    long = _prompts(model, (250, 3, 3), seed=44)        # max_position_embeddings = 256: 250 + 7 - 1 fits, 250 + 8 - 1 does not
    model.score(long, [[1] * 7, [2], [3]])
    with pytest.raises(ValueError):
        model.score(long, [[1] * 8, [2], [3]])
    for bad in (21, -1, 1057):
        with pytest.raises(ValueError):
            model.score(prompts, ok, top_logprobs=bad)


def test_generate_against_score_within_the_oracle_bf16_error(oracle):
    """The bf16 GEMV decode with a KV cache against the GEMM prefill without one, on the greedy tokens of the engine test:
    d = max |lp_generate - lp_score| over the counted positions <= 2 e_bf16 + 1e-2, e_bf16 the same maximum between
    the CPU oracle in eager bf16 and in fp32, teacher-forced on those tokens."""
    from oracle.model import lm_forward
    model, cfg, params = oracle
    prompts = _prompts(model)
    out, gen = _gen(model, prompts, temperature=0.0, return_logprobs=True)
    toks = _rows(out, 0, N, LENS)
    sc = model.score(prompts, toks.tolist())
    d = float((gen.logprobs.double() - sc.logprobs.double()).abs().max())
    p16 = {k: v.to(BF16) for k, v in params.items()}
    wte = params["lm.transformer.wte.weight"]
    e = 0.0
    for b, p in enumerate(prompts):
        seq = torch.cat([p.float().cpu(), wte[toks[b, :-1]].to(BF16).float()], 0)[None]
        lp = []
        for prm, x in ((params, seq), (p16, seq.to(BF16))):
            lg = lm_forward(prm, cfg, inputs_embeds=x)["logits"][0, p.shape[0] - 1:].double()
            lp.append(torch.log_softmax(lg, -1).gather(1, toks[b][:, None])[:, 0])
        e = max(e, float((lp[0] - lp[1]).abs().max()))
    print(f"cross-path: d = {d:.4e}, e_bf16 = {e:.4e}, bound {2 * e + 1e-2:.4e}")
    assert d <= 2 * e + 1e-2, (d, e)
