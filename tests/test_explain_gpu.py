"""Explaining an answer (ABI 20; DESIGN.md "Explaining an answer"): Magma.score(key_scale=) and Magma.explain on the reduced
2-block model carrying the CPU oracle's seeded weights (adapters x 20, q_proj / k_proj x 4 so that attention is not uniform).

The CPU statement below restates oracle.model.attention_fwd with the scale on the fp32 score; with scale 1 it equals
oracle.model.lm_forward exactly (test_explain_cpu.py)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LENS = (5, 9, 2)
TARGETS = ([17, 4, 250], [999, 3], [8, 8, 61, 700])


# ------------------------------------------------------------------------------------------------------ the CPU statement
def attention_scaled(p, cfg, i, x, key_scale):
    """oracle.model.attention_fwd without a cache, the scores multiplied by key_scale [B, S] (fp32) before the causal mask."""
    from oracle.model import adapter_fwd, apply_rotary, attn_prefix, parallel_adapter_fwd
    B, S, d = x.shape
    H, Dh = cfg.n_head, cfg.head_dim
    ap = attn_prefix(cfg, i)
    q = F.linear(x, p[ap + "q_proj.weight"]).view(B, S, H, Dh)
    k = F.linear(x, p[ap + "k_proj.weight"]).view(B, S, H, Dh)
    v = F.linear(x, p[ap + "v_proj.weight"]).view(B, S, H, Dh)
    pos = torch.arange(S)
    q = apply_rotary(q, pos, cfg.rotary_dim).permute(0, 2, 1, 3)
    k = apply_rotary(k, pos, cfg.rotary_dim).permute(0, 2, 1, 3)
    v = v.permute(0, 2, 1, 3)
    scores = torch.matmul(q.float(), k.float().transpose(-1, -2)) / math.sqrt(Dh)
    scores = scores * key_scale.float()[:, None, None, :]
    mask = torch.arange(S)[None, :] <= torch.arange(S)[:, None]
    scores = torch.where(mask, scores, torch.finfo(scores.dtype).min)
    w = torch.softmax(scores, dim=-1).to(v.dtype)
    o = torch.matmul(w, v).permute(0, 2, 1, 3).reshape(B, S, d)
    o = F.linear(o, p[ap + "out_proj.weight"])
    if cfg.attn_adapter_hidden and cfg.attn_adapter_type == "normal":
        o = adapter_fwd(p, f"lm.transformer.h.{i}.attn.adapter.", o, cfg.adapter_act)
    elif cfg.attn_adapter_hidden:
        o = parallel_adapter_fwd(p, f"lm.transformer.h.{i}.attn.adapter.", f"lm.transformer.h.{i}.attn.adapter_scale", x, o,
                                 cfg.adapter_act)
    return o


def lm_forward_scaled(p, cfg, x, key_scale):
    """oracle.model.lm_forward (cache-less) with attention_scaled in every block -> logits."""
    from oracle.model import mlp_fwd
    for i in range(cfg.n_layer):
        h = f"lm.transformer.h.{i}."
        ln = F.layer_norm(x, (cfg.d_model,), p[h + "ln_1.weight"], p[h + "ln_1.bias"], cfg.ln_eps)
        x = attention_scaled(p, cfg, i, ln, key_scale) + mlp_fwd(p, cfg, i, ln) + x
    x = F.layer_norm(x, (cfg.d_model,), p["lm.transformer.ln_f.weight"], p["lm.transformer.ln_f.bias"], cfg.ln_eps)
    return F.linear(x, p["lm.lm_head.weight"], p["lm.lm_head.bias"])


def statement_logprobs(params, cfg, prompt, toks, key_scale, dtype):
    """log p(toks[j] | prompt, toks[:j]) of ONE row under the statement in ``dtype`` (eager), fp64 [n].  prompt (n, d) bf16 values;
    key_scale fp32 [n + len(toks) - 1]."""
    prm = params if dtype == torch.float32 else {k: v.to(dtype) for k, v in params.items()}
    wte = params["lm.transformer.wte.weight"]
    toks = torch.as_tensor(toks, dtype=torch.int64)
    seq = torch.cat([prompt.float().cpu(), wte[toks[:-1]].to(BF16).float()], 0)[None].to(dtype)
    lg = lm_forward_scaled(prm, cfg, seq, key_scale[None])[0, prompt.shape[0] - 1:].double()
    return torch.log_softmax(lg, -1).gather(1, toks[:, None])[:, 0]


def statement_relevance(params, cfg, prompt, toks, suppression, dtype):
    """Default units of one row: relevance [n] = loss under unit u - loss, loss = mean negative log-probability."""
    n, W = prompt.shape[0], prompt.shape[0] + len(toks) - 1
    loss = -statement_logprobs(params, cfg, prompt, toks, torch.ones(W), dtype).mean()
    rel = []
    for u in range(n):
        ks = torch.ones(W)
        ks[u] = 1.0 - suppression
        rel.append(-statement_logprobs(params, cfg, prompt, toks, ks, dtype).mean() - loss)
    return torch.stack(rel)


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def oracle(dev):
    from magma_amd.testing import build_reduced_magma
    from oracle.model import OracleConfig, attn_prefix, init_params
    cfg = OracleConfig.tiny(mlp_adapter_hidden=128, attn_adapter_hidden=0)
    params = init_params(cfg, seed=11)
    for k in params:
        if ".adapter." in k:
            params[k] = params[k] * 20
    for i in range(cfg.n_layer):
        for w in ("q_proj.weight", "k_proj.weight"):
            params[attn_prefix(cfg, i) + w] = params[attn_prefix(cfg, i) + w] * 4
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


def _width(lens=LENS, targets=TARGETS):
    return max(n + len(t) - 1 for n, t in zip(lens, targets))


# --------------------------------------------------------------------------------------------------------------------- (g)
def test_score_with_key_scale_against_the_cpu_statement(oracle):
    """d = max |lp_gpu - lp_fp32| over the targets <= 2 e_bf16 + 1e-2, e_bf16 the same maximum between the statement in eager
    bf16 and in fp32 (the rule of test_generate_against_score_within_the_oracle_bf16_error)."""
    model, cfg, params = oracle
    prompts = _prompts(model)
    W = _width()
    g = torch.Generator().manual_seed(5)
    ks = torch.ones(len(LENS), W)
    for b, n in enumerate(LENS):
        ks[b, :n] = torch.rand(n, generator=g)
    got = model.score(prompts, [list(t) for t in TARGETS], key_scale=ks)
    d = e = 0.0
    for b, (p, t) in enumerate(zip(prompts, TARGETS)):
        w = p.shape[0] + len(t) - 1
        lp32 = statement_logprobs(params, cfg, p, t, ks[b, :w], torch.float32)
        lp16 = statement_logprobs(params, cfg, p, t, ks[b, :w], BF16)
        d = max(d, float((got.logprobs[b, : len(t)].double() - lp32).abs().max()))
        e = max(e, float((lp16 - lp32).abs().max()))
    print(f"score(key_scale): d = {d:.4e}, e_bf16 = {e:.4e}, bound {2 * e + 1e-2:.4e}")
    assert d <= 2 * e + 1e-2, (d, e)
    # the (B, S_prompt) form is the (B, W) form right-padded with 1.0
    short = model.score(prompts, [list(t) for t in TARGETS], key_scale=ks[:, : max(LENS)])
    assert torch.equal(short.logprobs, got.logprobs)


# --------------------------------------------------------------------------------------------------------------------- (h)
def test_scale_one_changes_nothing(model, monkeypatch):
    monkeypatch.setenv("MAGMA_ATTN_FWD", "5")
    prompts = _prompts(model)
    tg = [list(t) for t in TARGETS]
    base = model.score(prompts, tg, top_logprobs=3)
    ones = model.score(prompts, tg, top_logprobs=3, key_scale=torch.ones(len(LENS), _width()))
    for a, b in zip(base, ones):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------------------- (i)
UNITS = ([[0, 1], [2], [3, 4]], [[0, 1, 2, 3], [4, 5, 6, 7, 8]], [[1], [0]])


@pytest.mark.parametrize("batch_size", (4, 16))
@pytest.mark.parametrize("kind", ("positions", "groups", "similar"))
def test_explain_equals_its_host_statement(model, batch_size, kind):
    from magma_amd.sampling import explain_reference
    prompts = _prompts(model)
    tg = [list(t) for t in TARGETS]
    kw = dict(suppression=0.9, batch_size=batch_size, return_terms=True)
    if kind == "groups":
        kw["units"] = [[list(u) for u in row] for row in UNITS]
    if kind == "similar":
        kw["similarity_threshold"] = 0.0
    got, got_terms = model.explain(prompts, tg, **kw)
    ref, ref_terms = explain_reference(model, prompts, tg, **kw)
    for name, a, b in zip(got._fields, got, ref):
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert torch.equal(got_terms, ref_terms)
    n_units = [len(u) for u in UNITS] if kind == "groups" else list(LENS)
    assert got.count.tolist() == n_units and got.relevance.shape == (len(LENS), max(n_units))
    assert got.relevance.dtype == torch.float32 and got.loss.shape == (len(LENS),) and got.count.dtype == torch.int64
    for b, n in enumerate(n_units):
        assert bool((got.relevance[b, n:] == 0).all()) and bool((got.perturbed_loss[b, n:] == 0).all())
    for b, n in enumerate(n_units):
        assert torch.equal(got.relevance[b, :n], got.perturbed_loss[b, :n] - got.loss[b])
    assert float(got.relevance.abs().max()) > 0


# --------------------------------------------------------------------------------------------------------------------- (j)
def test_zero_suppression_is_exactly_zero(model):
    prompts = _prompts(model)
    out = model.explain(prompts, [list(t) for t in TARGETS], suppression=0.0, batch_size=4)
    assert torch.equal(out.relevance, torch.zeros(len(LENS), max(LENS)))
    for b, n in enumerate(LENS):
        assert torch.equal(out.perturbed_loss[b, :n], out.loss[b].expand(n))


# --------------------------------------------------------------------------------------------------------------------- (k)
def test_relevance_against_the_oracle(oracle):
    """One row, a 9-row prompt and 3 targets from torch.Generator().manual_seed(31), suppression 0.9:
    d_rel = max |relevance_gpu - relevance_fp32| <= 2 e_rel + 1e-2, e_rel the same maximum between the statement in eager bf16 and
    in fp32 -- and the precondition that makes this a test: max |relevance_fp32| >= 4 (2 e_rel + 1e-2).  On the CPU with these
    inputs: largest relevance 0.18, e_rel 0.006."""
    model, cfg, params = oracle
    g = torch.Generator().manual_seed(31)
    prompt = torch.randn(9, cfg.d_model, generator=g).to(BF16)
    toks = torch.randint(0, 1000, (3,), generator=g).tolist()
    rel32 = statement_relevance(params, cfg, prompt, toks, 0.9, torch.float32)
    rel16 = statement_relevance(params, cfg, prompt, toks, 0.9, BF16)
    e_rel = float((rel16 - rel32).abs().max())
    bound = 2 * e_rel + 1e-2
    out = model.explain([prompt.to(model.device)], [toks], suppression=0.9)
    d_rel = float((out.relevance[0].double() - rel32).abs().max())
    print(f"explain: d_rel = {d_rel:.4e}, e_rel = {e_rel:.4e}, bound {bound:.4e}")
    print("relevance fp32:", [round(float(v), 4) for v in rel32])
    print("relevance gpu: ", [round(float(v), 4) for v in out.relevance[0]])
    assert float(rel32.abs().max()) >= 4 * bound, (float(rel32.abs().max()), bound)
    assert d_rel <= bound, (d_rel, e_rel)


# --------------------------------------------------------------------------------------------------------------------- (m)
def test_refusals_before_any_launch(model, monkeypatch):
    from magma_amd import ops
    prompts = _prompts(model)
    tg = [list(t) for t in TARGETS]
    W = _width()
    launched = []
    monkeypatch.setattr(ops, "attn_prefill_scaled", lambda *a, **k: launched.append("scaled"))
    monkeypatch.setattr(ops, "attn_prefill", lambda *a, **k: launched.append("plain"))
    ok = torch.ones(len(LENS), W)
    for bad in (ok.clone().index_put_((torch.tensor(1), torch.tensor(2)), torch.tensor(-0.5)),
                ok.clone().index_put_((torch.tensor(0), torch.tensor(0)), torch.tensor(float("nan"))),
                ok.clone().index_put_((torch.tensor(2), torch.tensor(1)), torch.tensor(float("inf"))),
                ok[:, : W - 2], ok[:2], ok[0], torch.ones(len(LENS), W, dtype=torch.int64)):
        with pytest.raises(ValueError):
            model.score(prompts, tg, key_scale=bad)
    with pytest.raises(ValueError):                              # a unit naming a target position (row 2 has 2 prompt rows) ...
        model.explain(prompts, tg, units=[[[0]], [[0]], [[2]]])
    with pytest.raises(ValueError):                              # ... a padding position, a negative one
        model.explain(prompts, tg, units=[[[0]], [[0]], [[8]]])
    with pytest.raises(ValueError):
        model.explain(prompts, tg, units=[[[-1]], [[0]], [[0]]])
    with pytest.raises(ValueError):
        model.explain(prompts, tg, units=[[[0]], [[0]]])
    with pytest.raises(NotImplementedError, match="past_key_values"):
        model.score(prompts, tg, key_scale=ok, past_key_values=object())
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            model.explain(prompts, tg, batch_size=bad)
    for bad in (-0.1, 1.5, float("nan"), "0.9"):
        with pytest.raises(ValueError):
            model.explain(prompts, tg, suppression=bad)
    eng = model.lm.engine
    monkeypatch.setattr(eng, "fp8_mode", "attn")
    monkeypatch.setattr(eng, "fp8_attn", True)
    with pytest.raises(NotImplementedError, match="fp8"):
        model.score(prompts, tg, key_scale=ok)
    with pytest.raises(NotImplementedError, match="fp8"):
        model.explain(prompts, tg)
    with pytest.raises(NotImplementedError, match="fp8"):
        eng.score(torch.zeros(1, 4, eng.d, dtype=BF16, device=model.device), torch.zeros(1, 4, dtype=torch.int64), key_scale=torch.ones(1, 4))
    assert not launched


def test_engine_refuses_key_scale_on_the_cached_paths(model):
    """_blocks_prefill with ``chunk`` or ``tree`` and a key_scale names the mode."""
    eng = model.lm.engine
    emb = torch.zeros(1, 4, eng.d, dtype=BF16, device=model.device)
    ks = torch.ones(1, 4, device=model.device)
    with pytest.raises(NotImplementedError, match="chunk"):
        eng._blocks_prefill(emb, None, chunk=True, key_scale=ks)
    with pytest.raises(NotImplementedError, match="tree"):
        eng._blocks_prefill(emb, None, chunk=True, tree=(None, None, None, 1), key_scale=ks)
