"""Models without an MLP adapter: attention-only adapters of every type and option, and no adapters at all (reference
magma/magma.py:111-120 adds each adapter only when adapter_config names it; adapter_config None gives none).  Every engine
path -- prefill, cached decode (GEMV step, tile-GEMM step of B > 16, captured graph, W8A16), fp8 inference, the training
forward / backward (bottom-block prefix-rows form, fp8) and freeze_lm: false -- against the fp32 oracle, under the
tolerance rules the rest of the suite states (tests/test_model_gpu.py, test_variants_gpu.py, test_train_gpu.py,
test_fp8_gpu.py)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# id -> (attention adapter type or None, activation, add_layernorm)
CASES = {"none": (None, "relu", False), "attn_normal": ("normal", "relu", False), "attn_parallel": ("parallel", "relu", False),
         "attn_scaled": ("scaled_parallel", "relu", False), "attn_ln_gelu": ("normal", "gelu_tanh", True)}
_ACTS = {"relu": torch.nn.ReLU, "gelu_tanh": functools.partial(torch.nn.GELU, approximate="tanh")}


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-20))


def bf16_params(p):
    return {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in p.items()}


def check(err_hip, err_bf16, what, floor=2e-3):
    assert err_hip <= 2.0 * err_bf16 + floor, f"{what}: HIP err {err_hip:.3e} vs eager-bf16 err {err_bf16:.3e}"


def _adapter_config(case):
    attn, act, ln = CASES[case]
    if attn is None:
        return None
    return {"attention": dict(adapter_type=attn, downsample_factor=8, add_layernorm=ln, activation=_ACTS[act])}


def _build(dev, case, **kw):
    from magma_amd.testing import build_reduced_magma
    return build_reduced_magma(dev, mlp_factor=None, adapter_config=_adapter_config(case), **kw)


def _params(case, seed, scale=20, **kw):
    """Oracle config + parameters; the adapter projections ``scale`` x the 1e-3 init so that their arithmetic shows in the outputs."""
    from oracle.model import OracleConfig, init_params
    attn, act, ln = CASES[case]
    cfg = OracleConfig.tiny(mlp_adapter_hidden=0, attn_adapter_hidden=64 if attn else 0, attn_adapter_type=attn or "normal",
                            adapter_act=act, adapter_layernorm=ln, **kw)
    p = init_params(cfg, seed=seed)
    lin = ("1.", "3.") if ln else ("0.", "2.")
    for k in p:
        if ".adapter." in k and k.split(".adapter.")[1].startswith(lin):
            p[k] = p[k] * scale
    return cfg, p


def _loaded(dev, case, params, **kw):
    model = _build(dev, case, **kw)
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing, unexpected)
    return model


def test_helpers_build_the_requested_adapters(dev):
    from magma_amd.adapters import AdapterWrapper, ParallelAdapterWrapper
    from magma_amd.language_model import MLP, SelfAttention
    for case, (attn, _, ln) in CASES.items():
        model = _build(dev, case)
        blk = model.lm.transformer.h[0]
        assert isinstance(blk.mlp, MLP) and not model.mlp_adapter_added
        assert model.attn_adapter_added == (attn is not None)
        if attn is None:
            assert isinstance(blk.attn, SelfAttention)
        elif attn == "normal":
            assert isinstance(blk.attn, AdapterWrapper) and (blk.attn.ln is not None) == ln
        else:
            assert isinstance(blk.attn, ParallelAdapterWrapper)
            assert torch.is_tensor(blk.attn.adapter_scale) == (attn == "scaled_parallel")
        trainable_lm = [n for n, p in model.lm.named_parameters() if p.requires_grad]
        assert all("adapter" in n for n in trainable_lm) and bool(trainable_lm) == (attn is not None)


# ------------------------------------------------------------------------------------------------- a. inference vs the oracle
@pytest.mark.parametrize("case", list(CASES))
def test_inference_vs_oracle(dev, case):
    """Prefill, 4 cached steps and the full-sequence forward against the oracle."""
    from oracle.model import generate_greedy, lm_forward
    # a 'normal' attention adapter without LayerNorm reads the attention output (rows of norm ~0.1 x a LayerNorm output's):
    # larger projections there, so that the adapter moves the logits by the 2e-2 asserted below
    cfg, p = _params(case, seed=5, scale=60 if case == "attn_normal" else 20)
    model = _loaded(dev, case, p)
    model.eval()
    lm = {k: v for k, v in p.items() if k.startswith("lm.")}
    lmb = bf16_params(lm)
    g = torch.Generator().manual_seed(2)
    emb = torch.randn(2, 10, cfg.d_model, generator=g).to(torch.bfloat16).float()
    steps = 4
    with torch.no_grad():
        ref_toks, ref_logits = generate_greedy(lm, cfg, emb, steps, stop_on_eos=False)
        _, bf_logits = generate_greedy(lmb, cfg, emb.to(torch.bfloat16), steps, stop_on_eos=False)
        if CASES[case][0] is not None:       # the adapters must matter for this test to mean anything
            up = "3.weight" if CASES[case][2] else "2.weight"
            off = {k: (torch.zeros_like(v) if ".adapter." in k and k.endswith(up) else v) for k, v in lm.items()}
            assert rel(lm_forward(off, cfg, inputs_embeds=emb)["logits"], lm_forward(lm, cfg, inputs_embeds=emb)["logits"]) > 2e-2
        out = model.lm(inputs_embeds=emb.to(torch.bfloat16).cuda(), use_cache=True, cache_hint=steps)
        assert rel(out.logits[:, -1], ref_logits[0]) <= 2 * rel(bf_logits[0], ref_logits[0]) + 2e-3
        cache, S0 = out.past_key_values, emb.shape[1]
        for i in range(1, steps):
            o = model.lm(input_ids=ref_toks[:, S0 + i - 1: S0 + i].cuda(), use_cache=True, past_key_values=cache)
            assert rel(o.logits[:, -1], ref_logits[i]) <= 2 * max(rel(bf_logits[i], ref_logits[i]), 5e-3) + 2e-3, i
        full = model.lm(inputs_embeds=emb.to(torch.bfloat16).cuda())
        assert rel(full.logits, lm_forward(lm, cfg, inputs_embeds=emb)["logits"]) < 2e-2


# ------------------------------------------------------------------------------------------------- b. decode-step forms
@pytest.mark.parametrize("case", ["none", "attn_normal"])
def test_graph_decode_equals_eager(dev, case):
    """The captured decode step gives the eager step's logits and tokens bit for bit; generate() picks the same tokens."""
    cfg, p = _params(case, seed=11)
    model = _loaded(dev, case, p)
    model.eval()
    g = torch.Generator().manual_seed(5)
    images = torch.randn(2, 3, 64, 64, generator=g)
    ids = torch.randint(0, 1000, (2, 6), generator=g)
    emb = model.embed([images, ids])
    eng = model.lm.engine
    runs = {}
    with torch.no_grad():
        for use_graph in (False, True):
            out = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=6)
            toks, logits = [out.logits[:, -1].argmax(-1)], []
            cache = out.past_key_values
            for _ in range(5):
                lg, tk = eng.decode(toks[-1][:, None], cache, use_graph=use_graph)
                logits.append(lg.clone())
                toks.append(tk.clone())
            runs[use_graph] = (torch.stack(toks, 1), torch.stack(logits, 1))
        a = model.generate(emb, max_steps=6, temperature=0.0, decode=False, stop_on_eos=False)
    assert torch.equal(runs[True][1], runs[False][1])
    assert torch.equal(runs[True][0], runs[False][0])
    assert a.shape == (2, emb.shape[1] + 6) and torch.equal(a[:, emb.shape[1]:], runs[False][0])


@pytest.mark.parametrize("case", ["none", "attn_normal"])
def test_decode_batch_above_16(dev, case):
    """B = 24: prefill and 3 cached steps of the tile-GEMM token step against the oracle."""
    from oracle.model import lm_forward
    cfg, p = _params(case, seed=13)
    model = _loaded(dev, case, p)
    model.eval()
    lm = {k: v for k, v in p.items() if k.startswith("lm.")}
    lmb = bf16_params(lm)
    B, S0 = 24, 9
    g = torch.Generator().manual_seed(31)
    emb = torch.randn(B, S0, cfg.d_model, generator=g).to(torch.bfloat16).float()
    with torch.no_grad():
        r = lm_forward(lm, cfg, inputs_embeds=emb)
        rb = lm_forward(lmb, cfg, inputs_embeds=emb.to(torch.bfloat16))
        out = model.lm(inputs_embeds=emb.to(torch.bfloat16).cuda(), use_cache=True, cache_hint=8)
        check(rel(out.logits[:, -1], r["logits"][:, -1]), rel(rb["logits"][:, -1], r["logits"][:, -1]), "B=24 prefill")
        past, pastb, cache = r["past_key_values"], rb["past_key_values"], out.past_key_values
        tok = r["logits"][:, -1].argmax(-1, keepdim=True)
        for i in range(3):
            r = lm_forward(lm, cfg, input_ids=tok, past=past)
            rb = lm_forward(lmb, cfg, input_ids=tok, past=pastb)
            o = model.lm(input_ids=tok.cuda(), use_cache=True, past_key_values=cache)
            ref = r["logits"][:, -1]
            check(rel(o.logits[:, -1], ref), rel(rb["logits"][:, -1], ref), f"B=24 cached step {i}")
            top2 = torch.topk(ref, 2, dim=-1).values
            safe = (top2[:, 0] - top2[:, 1]) > 0.05 * ref.std(dim=-1)
            assert bool((o.next_token.cpu()[safe] == ref.argmax(-1)[safe]).all())
            past, pastb = r["past_key_values"], rb["past_key_values"]
            tok = ref.argmax(-1, keepdim=True)


# ------------------------------------------------------------------------------------------------- c. fp8 inference
@pytest.mark.parametrize("mode", ["attn", "all"])
@pytest.mark.parametrize("case", list(CASES))
def test_fp8_forward_stays_close_to_bf16(dev, case, mode):
    """Bounds of test_fp8_gpu.py::test_model_forward_in_fp8_stays_close_to_bf16: rel-L2 of the logits <= 0.1, |loss
    difference| <= 0.05 nats, and not bit-equal (the fp8 path was taken)."""
    torch.manual_seed(3)
    model = _build(dev, case)
    model.eval()
    g = torch.Generator().manual_seed(5)
    images = torch.randn(2, 3, 64, 64, generator=g).to(dev)
    caps = torch.randint(0, 1000, (2, model.seq_len), generator=g).to(dev)
    caps[:, 12:] = model.eos_token
    eng = model.lm.engine
    with torch.no_grad():
        ref = model(images, caps)
        emb = model.embed([images, caps[:, :6].contiguous()])
        ref_logits = model.lm(inputs_embeds=emb).logits.float()
        eng.fp8_mode = mode
        try:
            got = model(images, caps)
            got_logits = model.lm(inputs_embeds=emb).logits.float()
        finally:
            eng.fp8_mode = None
    assert torch.isfinite(got_logits).all()
    assert rel(got_logits, ref_logits) < 0.1, rel(got_logits, ref_logits)
    assert abs(float(got.loss) - float(ref.loss)) < 0.05, (float(got.loss), float(ref.loss))
    assert not torch.equal(got_logits, ref_logits), "fp8 mode did not change anything: the fp8 path was not taken"


@pytest.mark.parametrize("case", ["none", "attn_normal"])
def test_w8a16_generate_tracks_bf16(dev, case):
    """Full-width 2-block model (d = 4096, full vocabulary), rules of test_fp8_gpu.py::test_w8a16_generate_tracks_bf16:
    rel-L2 of the step logits <= 0.08, identical tokens where the bf16 top-1 margin is clear, not bit-equal."""
    from magma_amd import Magma
    from magma_amd.image_encoders import ModifiedResNetTrunk
    from magma_amd.language_model import GPTJConfig
    from magma_amd.testing import tiny_multimodal_config
    torch.manual_seed(7)
    enc = ModifiedResNetTrunk((1, 1, 2, 1), 16, 64, device=dev, dtype=torch.bfloat16)
    cfg = tiny_multimodal_config(mlp_factor=None, adapter_config=_adapter_config(case))
    model = Magma(cfg, device=dev, lm_config=GPTJConfig(num_layers=2, vocab_size=50258), enc=enc)
    model.eval()
    assert model.lm.config.hidden_size == 4096
    eng = model.lm.engine
    g = torch.Generator(device=dev).manual_seed(3)
    images = torch.randn(8, 3, 64, 64, device=dev, generator=g).to(torch.bfloat16)
    prompt = torch.randint(0, 50256, (8, 8), device=dev, generator=g)
    with torch.no_grad():
        emb = model.embed([images, prompt])
        logits = {}
        for mode in (False, True):
            eng.decode_w8 = mode
            eng._cache_pool.clear()
            pre = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=8)
            tok = pre.logits[:, -1].argmax(-1, keepdim=True)
            step = model.lm(input_ids=tok, use_cache=True, past_key_values=pre.past_key_values)
            logits[mode] = step.logits[:, -1].float().clone()
        eng.decode_w8 = False
        eng._cache_pool.clear()
    assert rel(logits[True], logits[False]) < 0.08, rel(logits[True], logits[False])
    top2 = logits[False].topk(2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 0.2 * logits[False].std(dim=-1)
    assert bool((logits[True].argmax(-1)[clear] == logits[False].argmax(-1)[clear]).all())
    assert not torch.equal(logits[True], logits[False])


# ------------------------------------------------------------------------------------------------- d. training gradients
def _batch(cfg, S, seed):
    g = torch.Generator().manual_seed(seed)
    B = 2
    images = torch.randn(B, 3, 64, 64, generator=g)
    caps = torch.full((B, S), cfg.eos_token, dtype=torch.int64)
    caps[0, :23] = torch.randint(0, 1000, (23,), generator=g)
    caps[1, :11] = torch.randint(0, 1000, (11,), generator=g)
    mask = (torch.rand(B, 4, cfg.d_model, generator=g) < 0.9).float() / 0.9
    return images, caps, mask


def _oracle_grads(cfg, params, images, caps, mask, dtype):
    from oracle.model import magma_forward
    p = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v) for k, v in params.items()}
    names = [k for k in p if (".adapter." in k or "adapter_scale" in k or k.startswith("image_prefix.")) and "running_" not in k]
    for k in names:
        p[k].requires_grad_(True)
    out = magma_forward(p, cfg, images.to(dtype), caps, dropout_mask=mask.to(dtype))
    out["loss"].backward()
    return float(out["loss"]), {k: p[k].grad.float() for k in names}


def _engine_grads(dev, case, params, images, caps, mask):
    from magma_amd.train_engine import MagmaEngine
    model = _loaded(dev, case, params, n_positions=128)
    model.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(model)
    eng.train()
    out = eng(images.to(dev), caps.to(dev), dropout_mask=mask.to(dev))
    eng.backward(out.loss)
    name_of = {id(p): n for n, p in model.named_parameters()}
    grads = {}
    for grp in eng.groups:
        for p in grp.params:
            n = name_of[id(p)]
            grads["lm." + n if n.startswith("transformer.") else n] = eng.grad_of(p).float().cpu().clone()
    return eng, float(out.loss), grads


@pytest.mark.parametrize("case", list(CASES))
def test_train_gradients_vs_oracle(dev, case, monkeypatch):
    """Gradient of every trainable tensor from the explicit HIP backward against autograd through the fp32 oracle:
    err(HIP) <= 2 x err(bf16 autograd) + 3e-2 per tensor (the adapter_scale scalars judged together as one vector), global
    cosine > 0.999, the same set of trainable tensors.  The bottom block forms its input gradient for the prefix rows only
    (parallel adapters excepted: their input gradient reaches every row of ln_1, train_engine._lm_backward); for none and
    attn_normal the all-rows form gives bit-identical adapter gradients and prefix / trunk gradients within the criterion."""
    from magma_amd import train_engine
    cfg, params = _params(case, seed=23, n_positions=128)
    images, caps, mask = _batch(cfg, 128, seed=3)
    loss_ref, g_ref = _oracle_grads(cfg, params, images, caps, mask, torch.float32)
    loss_bf, g_bf = _oracle_grads(cfg, params, images, caps, mask, torch.bfloat16)
    if case == "none":
        assert g_ref and all(k.startswith("image_prefix.") for k in g_ref)
    monkeypatch.setattr(train_engine, "_BOTTOM_PREFIX_ONLY", True)
    eng, loss, grads = _engine_grads(dev, case, params, images, caps, mask)
    assert abs(loss - loss_ref) <= 2 * abs(loss_bf - loss_ref) + 3e-3 * abs(loss_ref), (loss, loss_ref, loss_bf)
    assert set(grads) == set(g_ref), (set(grads) ^ set(g_ref))
    parallel = CASES[case][0] in ("parallel", "scaled_parallel")
    assert eng.bottom_prefix_rows == (0 if parallel else 4), eng.bottom_prefix_rows
    dots = n1 = n2 = 0.0
    bad, scal = [], []
    for n, ref in g_ref.items():
        got, ref = grads[n].reshape(-1), ref.reshape(-1)
        e_hip, e_bf = rel(got, ref), rel(g_bf[n].reshape(-1), ref)
        if "adapter_scale" in n:
            scal.append((float(got), float(ref), float(g_bf[n])))
        elif e_hip > 2 * e_bf + 3e-2:
            bad.append((n, e_hip, e_bf))
        dots += float((got * ref).sum()); n1 += float((got * got).sum()); n2 += float((ref * ref).sum())
    assert not bad, bad
    assert bool(scal) == (case == "attn_scaled")
    if scal:
        t = torch.tensor(scal)
        e_hip, e_bf = rel(t[:, 0], t[:, 1]), rel(t[:, 2], t[:, 1])
        assert e_hip <= 2 * e_bf + 3e-2, (e_hip, e_bf, scal)
    assert dots / (n1 ** 0.5 * n2 ** 0.5) > 0.999
    eng.step()
    eng.eval()
    assert torch.isfinite(eng(images.to(dev), caps.to(dev)).loss)
    if case not in ("none", "attn_normal"):
        return
    monkeypatch.setattr(train_engine, "_BOTTOM_PREFIX_ONLY", False)
    eng_off, _, g_off = _engine_grads(dev, case, params, images, caps, mask)
    assert eng_off.bottom_prefix_rows == 0
    bad = []
    for n, ref in g_ref.items():
        if ".adapter." in n:
            assert torch.equal(grads[n], g_off[n]), n
        e_off, e_bf = rel(g_off[n], ref), rel(g_bf[n], ref)
        if e_off > 2 * e_bf + 3e-2:
            bad.append((n, e_off, e_bf))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------- e. fp8 training
@pytest.mark.parametrize("case", ["none", "attn_normal"])
def test_fp8_training_tracks_bf16(dev, case):
    """Rules of test_fp8_gpu.py::test_training_step_in_fp8_tracks_bf16: |loss difference| <= 0.02, gradient cosine >= 0.98,
    weights packed for fp8, not bit-equal."""
    from magma_amd.train_engine import MagmaEngine
    grads, losses = {}, {}
    for mode in (False, True):
        torch.manual_seed(11)
        model = _build(dev, case, n_positions=128)
        model.config.gradient_accumulation_steps = 1
        eng = MagmaEngine(model)
        eng.fp8 = mode
        eng.train()
        g = torch.Generator().manual_seed(3)
        B, S = 2, model.seq_len
        images = torch.randn(B, 3, 64, 64, generator=g).to(dev)
        caps = torch.full((B, S), model.eos_token, dtype=torch.int64)
        caps[0, :23] = torch.randint(0, 1000, (23,), generator=g)
        caps[1, :11] = torch.randint(0, 1000, (11,), generator=g)
        mask = ((torch.rand(B, 4, model.lm.config.hidden_size, generator=g) < 0.9).float() / 0.9).to(dev)
        out = eng(images, caps.to(dev), dropout_mask=mask)
        eng.backward(out.loss)
        losses[mode] = float(out.loss)
        grads[mode] = torch.cat([grp.grad.float().flatten() for grp in eng.groups]).clone()
        if mode:
            assert eng._fp8_packs, "fp8 mode did not pack any weight: the fp8 path was not taken"
    assert abs(losses[True] - losses[False]) < 0.02, losses
    a, b = grads[True], grads[False]
    cos = float((a * b).sum() / (a.norm() * b.norm()))
    assert cos > 0.98, cos
    assert not torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- f. freeze_lm: false
def test_freeze_lm_false_without_adapters(dev):
    """Plain fine-tuning of GPT-J plus the image prefix: every tensor's gradient against autograd through the fp32 oracle,
    criterion of test_train_gpu.py::test_freeze_lm_false_trains_every_gptj_tensor; then a step and a forward on the updated LM."""
    from magma_amd.train_engine import MagmaEngine
    from oracle.model import magma_forward
    cfg, params = _params("none", seed=27, n_positions=128)
    model = _loaded(dev, "none", params, n_positions=128)
    model.config.freeze_lm = False
    for p in model.lm.parameters():
        p.requires_grad = True
    model.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(model)
    eng.train()
    images, caps, mask = _batch(cfg, 128, seed=4)

    def oracle(dtype):
        p = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v) for k, v in params.items()}
        names = [k for k in p if p[k].is_floating_point() and "running_" not in k and "num_batches" not in k]
        for k in names:
            p[k].requires_grad_(True)
        out = magma_forward(p, cfg, images.to(dtype), caps, dropout_mask=mask.to(dtype))
        out["loss"].backward()
        return float(out["loss"].detach()), {k: p[k].grad.float() for k in names if p[k].grad is not None}

    loss_ref, g_ref = oracle(torch.float32)
    loss_bf, g_bf = oracle(torch.bfloat16)
    out = eng(images.to(dev), caps.to(dev), dropout_mask=mask.to(dev))
    assert abs(float(out.loss) - loss_ref) <= 2 * abs(loss_bf - loss_ref) + 3e-3 * abs(loss_ref)
    eng.backward(out.loss)
    name_of = {id(p): n for n, p in model.named_parameters()}
    seen, bad = set(), []
    for grp in eng.groups:
        for p in grp.params:
            n = name_of[id(p)]
            n = "lm." + n if n.startswith("transformer.") else ("lm.transformer.wte.weight" if n == "word_embedding.weight" else n)
            if n in seen or n not in g_ref:
                continue
            seen.add(n)
            e_hip, e_bf = rel(eng.grad_of(p), g_ref[n]), rel(g_bf[n], g_ref[n])
            if e_hip > 2 * e_bf + 3e-2:
                bad.append((n, e_hip, e_bf))
    missing = set(g_ref) - seen
    assert not missing, sorted(missing)[:10]
    assert any("q_proj" in n for n in seen) and any("lm_head" in n for n in seen) and any("wte" in n for n in seen)
    assert not any("adapter" in n for n in seen)
    assert not bad, bad[:8]
    qw = model.lm.transformer.h[0].attn.attention.q_proj.weight
    before = eng.master_of(qw).clone()
    eng.step()
    out2 = eng(images.to(dev), caps.to(dev), dropout_mask=mask.to(dev))
    assert torch.isfinite(out2.loss)
    eng.backward(out2.loss)
    eng.step()
    assert float((eng.master_of(qw) - before).abs().max()) > 0
    eng.eval()
    assert torch.isfinite(eng(images.to(dev), caps.to(dev)).loss)
