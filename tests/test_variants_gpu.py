"""Model variants and reference-surface leftovers of SURVEY 8f row 4 / VERDICT r1: parallel and scaled_parallel
adapters (reference magma/adapters.py:42-92, magma/magma.py:129-136,154-161) against the oracle (itself pinned to the
reference classes run in place, tests/test_oracle_pins.py), Adapter used as a stand-alone module, the RN50x4 trunk,
Magma.from_checkpoint as a classmethod on a DeepSpeed-layout file, forward(...).logits, the ``magma`` import path."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def bf16_params(p):
    return {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in p.items()}


def _build(dev, mlp_type, attn_type):
    from magma_amd.config import MultimodalConfig
    from magma_amd.image_encoders import ModifiedResNetTrunk
    from magma_amd.language_model import GPTJConfig
    from magma_amd.magma import Magma
    ad = {"mlp": {"adapter_type": mlp_type, "downsample_factor": 4}}
    if attn_type:
        ad["attention"] = {"adapter_type": attn_type, "downsample_factor": 8}
    cfg = MultimodalConfig(batch_size=2, train_steps=1, encoder_name="clip_resnet_large", adapter_config=ad, image_size=64,
                           freeze_img_encoder=False, use_image_embed_layernorm=True, image_embed_dropout_prob=0.1)
    lm_cfg = GPTJConfig(vocab_size=1056, hidden_size=512, num_layers=2, num_heads=2, rotary_dim=64, intermediate_size=2048,
                        max_position_embeddings=256)
    enc = ModifiedResNetTrunk((1, 1, 2, 1), 16, 64, device=dev, dtype=torch.bfloat16)
    return Magma(cfg, device=dev, lm_config=lm_cfg, enc=enc)


@pytest.mark.parametrize("mlp_type,attn_type", [("parallel", None), ("scaled_parallel", "scaled_parallel"),
                                                ("normal", "parallel")])
def test_parallel_adapters_vs_oracle(dev, mlp_type, attn_type):
    from oracle.model import OracleConfig, generate_greedy, init_params, lm_forward
    cfg = OracleConfig.tiny(mlp_adapter_hidden=128, attn_adapter_hidden=64 if attn_type else 0,
                            mlp_adapter_type=mlp_type, attn_adapter_type=attn_type or "normal")
    p = init_params(cfg, seed=5)
    for k in p:
        if ".adapter." in k:
            p[k] = p[k] * 20
    model = _build(dev, mlp_type, attn_type)
    missing, unexpected = model.load_checkpoint_state(p)           # reference key names: mlp.module.*, mlp.adapter.*, adapter_scale
    assert not unexpected and not missing, (missing, unexpected)
    model.eval()
    lm, lmb = {k: v for k, v in p.items() if k.startswith("lm.")}, None
    lmb = bf16_params(lm)
    g = torch.Generator().manual_seed(2)
    emb = torch.randn(2, 10, cfg.d_model, generator=g).to(torch.bfloat16).float()
    steps = 4
    with torch.no_grad():
        ref_toks, ref_logits = generate_greedy(lm, cfg, emb, steps, stop_on_eos=False)
        _, bf_logits = generate_greedy(lmb, cfg, emb.to(torch.bfloat16), steps, stop_on_eos=False)
        # the adapters must matter for this test to mean anything
        off = dict(lm)
        for k in off:
            if ".adapter." in k and k.endswith("2.weight"):
                off[k] = torch.zeros_like(off[k])
        assert rel(lm_forward(off, cfg, inputs_embeds=emb)["logits"], lm_forward(lm, cfg, inputs_embeds=emb)["logits"]) > 2e-2
        out = model.lm(inputs_embeds=emb.to(torch.bfloat16).cuda(), use_cache=True, cache_hint=steps)
        assert rel(out.logits[:, -1], ref_logits[0]) <= 2 * rel(bf_logits[0], ref_logits[0]) + 2e-3
        cache, S0 = out.past_key_values, emb.shape[1]
        for i in range(1, steps):
            o = model.lm(input_ids=ref_toks[:, S0 + i - 1: S0 + i].cuda(), use_cache=True, past_key_values=cache)
            assert rel(o.logits[:, -1], ref_logits[i]) <= 2 * max(rel(bf_logits[i], ref_logits[i]), 5e-3) + 2e-3, i
        # full-sequence path
        full = model.lm(inputs_embeds=emb.to(torch.bfloat16).cuda())
        assert rel(full.logits, lm_forward(lm, cfg, inputs_embeds=emb)["logits"]) < 2e-2


@pytest.mark.parametrize("mlp_type,attn_type", [("parallel", None), ("scaled_parallel", "scaled_parallel")])
def test_parallel_adapters_train_gradients(dev, mlp_type, attn_type):
    """Training with parallel / scaled_parallel adapters: gradients of every trainable tensor (adapter weights and biases,
    the adapter_scale scalars, prefix, trunk) from the explicit HIP backward against autograd through the fp32 oracle.
    Tolerance as tests/test_train_gpu.py: err(HIP) <= 2 x err(bf16 autograd) + 3e-2 per tensor, cosine > 0.999."""
    from magma_amd.train_engine import MagmaEngine
    from oracle.model import OracleConfig, init_params, magma_forward
    cfg = OracleConfig.tiny(mlp_adapter_hidden=128, attn_adapter_hidden=64 if attn_type else 0,
                            mlp_adapter_type=mlp_type, attn_adapter_type=attn_type or "normal")
    params = init_params(cfg, seed=23)
    for k in params:
        if ".adapter." in k:
            params[k] = params[k] * 20
    model = _build(dev, mlp_type, attn_type)
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing, unexpected)
    model.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(model)
    eng.train()
    g = torch.Generator().manual_seed(3)
    B, S = 2, model.seq_len
    images = torch.randn(B, 3, 64, 64, generator=g)
    caps = torch.full((B, S), cfg.eos_token, dtype=torch.int64)
    caps[0, :23] = torch.randint(0, 1000, (23,), generator=g)
    caps[1, :11] = torch.randint(0, 1000, (11,), generator=g)
    mask = (torch.rand(B, 4, cfg.d_model, generator=g) < 0.9).float() / 0.9

    def oracle_grads(dtype):
        p = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v) for k, v in params.items()}
        names = [k for k in p if (".adapter." in k or "adapter_scale" in k or k.startswith("image_prefix.")) and "running_" not in k]
        for k in names:
            p[k].requires_grad_(True)
        out = magma_forward(p, cfg, images.to(dtype), caps, dropout_mask=mask.to(dtype))
        out["loss"].backward()
        return float(out["loss"]), {k: p[k].grad.float() for k in names}

    loss_ref, g_ref = oracle_grads(torch.float32)
    loss_bf, g_bf = oracle_grads(torch.bfloat16)
    out = eng(images.to(dev), caps.to(dev), dropout_mask=mask.to(dev))
    assert abs(float(out.loss) - loss_ref) <= 2 * abs(loss_bf - loss_ref) + 3e-3 * abs(loss_ref)
    eng.backward(out.loss)
    name_of = {id(p): n for n, p in model.named_parameters()}
    dots = n1 = n2 = 0.0
    seen = set()
    bad, scal = [], []
    for grp in eng.groups:
        for p in grp.params:
            n = name_of[id(p)]
            n = "lm." + n if n.startswith("transformer.") else n
            if n in seen or n not in g_ref:
                continue
            seen.add(n)
            got, ref = eng.grad_of(p).float().cpu().reshape(-1), g_ref[n].reshape(-1)
            e_hip, e_bf = rel(got, ref), rel(g_bf[n].reshape(-1), ref)
            if "adapter_scale" in n:      # scalars (a sum of 260k signed products each): judged together as one vector below
                scal.append((float(got), float(ref), float(g_bf[n])))
            elif e_hip > 2 * e_bf + 3e-2:
                bad.append((n, e_hip, e_bf))
            dots += float((got * ref).sum()); n1 += float((got * got).sum()); n2 += float((ref * ref).sum())
    assert not bad, bad
    if scal:
        t = torch.tensor(scal)
        e_hip, e_bf = rel(t[:, 0], t[:, 1]), rel(t[:, 2], t[:, 1])
        print("adapter_scale gradients (hip, fp32 oracle, bf16 oracle):", scal)
        assert e_hip <= 2 * e_bf + 3e-2, (e_hip, e_bf, scal)
    assert len(seen) == len(g_ref), set(g_ref) - seen
    assert any("adapter_scale" in n for n in seen) == (mlp_type == "scaled_parallel")
    assert dots / (n1 ** 0.5 * n2 ** 0.5) > 0.999
    eng.step()                                   # the step runs, and the inference engine sees the new scale afterwards
    eng.eval()
    assert torch.isfinite(eng(images.to(dev), caps.to(dev)).loss)


def test_adapter_as_a_module(dev):
    """reference adapters.py:38-39: Adapter.forward(x) = adapter(x) + x, callable on its own."""
    from magma_amd.adapters import Adapter
    from oracle.model import adapter_fwd
    torch.manual_seed(0)
    ad = Adapter(dim=512, downsample_factor=4, device=dev, dtype=torch.bfloat16)
    with torch.no_grad():
        for m in (ad.adapter[0], ad.adapter[2]):
            m.weight.mul_(30)
    x = torch.randn(3, 7, 512, device=dev).to(torch.bfloat16)
    y = ad(x)
    p = {"a." + k.replace("adapter.", ""): v.float().cpu() for k, v in ad.state_dict().items()}
    ref = adapter_fwd(p, "a.", x.float().cpu())
    assert y.shape == x.shape and rel(y, ref) < 4e-3
    assert rel(y - x, ref - x.float().cpu()) < 2e-2          # the adapter branch itself, not just the residual
    # the packed operands are cached: a second call with unchanged parameters re-uses them
    packs = ad.__dict__["_pack_cache"]
    ad(x)
    assert ad.__dict__["_pack_cache"] is packs
    # an ordinary in-place update (what torch optimizers do: _version moves) is seen by itself
    with torch.no_grad():
        ad.adapter[2].bias.add_(0.25)
    y1 = ad(x)
    assert ad.__dict__["_pack_cache"] is not packs and rel(y1, ref) > 1e-2
    # parameters rewritten behind autograd's back -- what the engines' raw-pointer AdamW does (no _version bump, same data_ptr):
    # such writers bump the weights epoch (train_engine._step_impl, Magma.invalidate_packed), and the next call computes with the
    # NEW values
    from magma_amd.adapters import bump_weights_epoch
    ad.adapter[0].weight.data.mul_(0.5)
    bump_weights_epoch()
    y2 = ad(x)
    p2 = {"a." + k.replace("adapter.", ""): v.float().cpu() for k, v in ad.state_dict().items()}
    ref2 = adapter_fwd(p2, "a.", x.float().cpu())
    assert rel(y2, ref2) < 4e-3 and rel(y2, ref) > 1e-2


def test_rn50x4_trunk(dev):
    """clip_resnet (RN50x4: layers (4,6,10,6), width 80 -> 2560 channels, reference image_encoders.py:58-59,
    image_prefix.py:19) through the same kernels, against the oracle's trunk at that geometry."""
    from magma_amd.image_encoders import get_image_encoder
    from oracle.model import OracleConfig, encoder_fwd, init_params
    cfg = OracleConfig(n_layer=0, vocab_in=8, vocab_out=8, enc_width=80, enc_layers=(4, 6, 10, 6))
    p = init_params(cfg, seed=1)
    enc = get_image_encoder("clip_resnet", device=dev, dtype=torch.bfloat16)
    assert enc.out_dim == 2560 and enc.input_resolution == 288
    sd = {k[len("image_prefix.enc."):]: v for k, v in p.items() if k.startswith("image_prefix.enc.")}
    enc.load_state_dict(sd, strict=False)
    enc.invalidate_packed()
    x = torch.randn(1, 3, 96, 96, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).float()
    with torch.no_grad():
        ref = encoder_fwd(p, cfg, x)
        eb = rel(encoder_fwd(bf16_params(p), cfg, x.to(torch.bfloat16)), ref)
        got = enc(x.cuda())
    assert got.shape == ref.shape == (1, 9, 2560)
    assert rel(got, ref) <= 2 * eb + 5e-3


def test_from_checkpoint_classmethod_and_logits(dev, tmp_path, monkeypatch):
    """Magma.from_checkpoint (reference magma.py:278-301) on a DeepSpeed-layout file {"module": state_dict} that carries the
    reference's duplicate keys (Q8: transformer.N... / word_embedding.weight) and the fork's attention buffers; then
    forward(...).logits (reference magma.py:270-276) on request."""
    from magma_amd import Magma
    from magma_amd.testing import build_reduced_magma, tiny_multimodal_config
    from magma_amd.language_model import GPTJConfig
    from magma_amd.image_encoders import ModifiedResNetTrunk
    from oracle.model import OracleConfig, init_params, magma_forward
    cfg = OracleConfig.tiny()
    p = init_params(cfg, seed=9)
    sd = dict(p)
    for k, v in p.items():                      # the aliases a real checkpoint carries
        if k.startswith("lm.transformer.h."):
            sd["transformer." + k[len("lm.transformer.h."):]] = v
    sd["word_embedding.weight"] = p["lm.transformer.wte.weight"]
    sd["lm.transformer.h.0.attn.attention.bias"] = torch.ones(1, 1, 8, 8)
    sd["lm.transformer.h.0.attn.attention.masked_bias"] = torch.tensor(-1e9)
    path = tmp_path / "mp_rank_00_model_states.pt"
    # DeepSpeed's mp_rank_00_model_states.pt carries non-tensor objects next to "module" (an argparse Namespace, numpy
    # scalars): the file needs the reference's full unpickle (magma.py:292), not torch 2.10's weights_only default
    import argparse
    import numpy as np
    torch.save({"module": sd, "global_steps": 3, "args": argparse.Namespace(lr=8e-4, config="MAGMA_v1.yml"),
                "skipped_steps": np.int64(0), "ds_version": "0.3.15"}, path)
    kw = dict(lm_config=GPTJConfig(vocab_size=1056, hidden_size=512, num_layers=2, num_heads=2, rotary_dim=64,
                                   intermediate_size=2048, max_position_embeddings=256),
              enc=ModifiedResNetTrunk((1, 1, 2, 1), 16, 64, device=dev, dtype=torch.bfloat16))
    monkeypatch.delenv("MAGMA_ALLOW_BYTE_TOKENIZER", raising=False)
    from magma_amd.tokenizer import ByteTokenizer, get_tokenizer
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        stand_in = isinstance(get_tokenizer("gpt2", 256), ByteTokenizer)
    if stand_in:        # no GPT-2 files on this box: trained weights + byte-level ids must be refused
        with pytest.raises(RuntimeError, match="tokenizer"):
            Magma.from_checkpoint(tiny_multimodal_config(), str(path), device=dev, **kw)
    monkeypatch.setenv("MAGMA_ALLOW_BYTE_TOKENIZER", "1")
    model = Magma.from_checkpoint(tiny_multimodal_config(), str(path), device=dev, **kw)
    assert not model.training
    g = torch.Generator().manual_seed(9)
    images = torch.randn(2, 3, 64, 64, generator=g)
    caps = torch.full((2, 256), cfg.eos_token, dtype=torch.int64)
    caps[0, :20] = torch.randint(0, 1000, (20,), generator=g)
    caps[1, :9] = torch.randint(0, 1000, (9,), generator=g)
    ref = magma_forward(p, cfg, images, caps)
    out = model(images.cuda(), caps.cuda(), return_logits=True)
    assert abs(float(out.loss) - float(ref["loss"])) < 1e-2 * abs(float(ref["loss"]))
    assert out.logits.shape == ref["logits"].shape and rel(out.logits, ref["logits"]) < 2e-2
    # default call, as the reference's (magma.py:238-276): .logits is there -- materialised on first access, not before
    from magma_amd.language_model import LMOutput
    o2 = model(images.cuda(), caps.cuda())
    assert isinstance(dict.__getitem__(o2, "logits"), LMOutput.lazy)
    assert o2.logits.shape == ref["logits"].shape and torch.equal(o2.logits, out.logits) and o2["logits"] is o2.logits
    # a checkpoint whose tensor shapes disagree with the model is an error, as load_state_dict(strict=False) makes it
    bad = dict(sd)
    bad["image_prefix.proj.weight"] = torch.zeros(7, 5)
    torch.save({"module": bad}, path)
    with pytest.raises(RuntimeError, match="size mismatch"):
        Magma.from_checkpoint(tiny_multimodal_config(), str(path), device=dev, **kw)


def test_magma_import_path(dev):
    """reference example_inference.py:1-2 / magma/__init__.py:1-20."""
    from magma import Magma, collate_fn, train_step  # noqa: F401
    from magma.image_input import ImageInput
    import magma_amd
    assert Magma is magma_amd.Magma and ImageInput is magma_amd.ImageInput


@pytest.mark.parametrize("geom", ["reduced", "vit_b32"])
def test_clip_vit_encoder_and_pooled_prefix(dev, geom):
    """encoder_name "clip" (ViT-B/32, reference image_encoders.py:56-63) + the pooled ImagePrefix branch (image_prefix.py:60-72,
    85-101) against the oracle (CLIP VisionTransformer restated and pinned to HF CLIPVisionModelWithProjection)."""
    from magma_amd.image_encoders import VisionTransformer
    from magma_amd.image_prefix import ImagePrefix
    from magma_amd.testing import tiny_multimodal_config
    from oracle.model import ViTConfig, init_vit_params, pooled_prefix_fwd, vit_encoder_fwd
    v = ViTConfig() if geom == "vit_b32" else ViTConfig(width=128, layers=2, heads=2, patch=8, resolution=32, out_dim=48)
    p = init_vit_params(v, seed=3)
    enc = VisionTransformer(v.resolution, v.patch, v.width, v.layers, v.heads, v.out_dim, device=dev, dtype=torch.bfloat16)
    sd = {k[len("image_prefix.enc."):]: t for k, t in p.items()}
    missing, unexpected = enc.load_state_dict(sd, strict=True), None
    enc.invalidate_packed()
    x = torch.randn(2, 3, v.resolution, v.resolution, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).float()
    with torch.no_grad():
        ref = vit_encoder_fwd(p, v, x)
        eb = rel(vit_encoder_fwd(bf16_params(p), v, x.to(torch.bfloat16)), ref)
        got = enc(x.cuda())
    assert got.shape == ref.shape == (2, v.out_dim)
    assert rel(got, ref) <= 2 * eb + 5e-3, (rel(got, ref), eb)
    # pooled prefix: Linear(out_dim -> seq_len * d) + "b (s d) -> b s d" + LayerNorm
    d, s = 512, 3
    cfg = tiny_multimodal_config(encoder_name="clip", image_seq_len=s, image_size=v.resolution)
    ip = ImagePrefix(cfg, out_dim=d, device=dev, dtype=torch.bfloat16, enc=enc)
    assert ip.pooled and ip.out_seq_len == s and ip.proj.weight.shape == (s * d, v.out_dim)
    g = torch.Generator().manual_seed(1)
    pp = dict(p)
    pp["image_prefix.proj.weight"] = torch.randn(s * d, v.out_dim, generator=g) * v.out_dim ** -0.5
    pp["image_prefix.proj.bias"] = torch.randn(s * d, generator=g) * 0.02
    pp["image_prefix.ln.weight"] = 1.0 + torch.randn(d, generator=g) * 0.05
    pp["image_prefix.ln.bias"] = torch.randn(d, generator=g) * 0.02
    with torch.no_grad():
        ip.proj.weight.copy_(pp["image_prefix.proj.weight"]); ip.proj.bias.copy_(pp["image_prefix.proj.bias"])
        ip.ln.weight.copy_(pp["image_prefix.ln.weight"]); ip.ln.bias.copy_(pp["image_prefix.ln.bias"])
    ip.invalidate_packed()
    ip.eval()
    with torch.no_grad():
        ref2 = pooled_prefix_fwd(pp, d, s, ref)
        ppb = bf16_params(pp)
        eb2 = rel(pooled_prefix_fwd(ppb, d, s, vit_encoder_fwd(ppb, v, x.to(torch.bfloat16))), ref2)
        got2 = ip(x.cuda())
    assert got2.shape == (2, s, d)
    assert rel(got2, ref2) <= 2 * eb2 + 5e-3, (rel(got2, ref2), eb2)


def test_vit_pooled_prefix_train_gradients(dev):
    """Training with encoder_name "clip" (CLIP ViT-B/32, all 12 blocks trainable) and the pooled image prefix: loss and the
    gradient of every trainable tensor -- patch conv, class / positional embedding, every LayerNorm, in_proj / out_proj /
    MLP weights and biases, the 512-d projection, prefix Linear + LayerNorm, LM adapters -- against autograd through the
    fp32 oracle (vit_encoder_fwd pinned to HF CLIP, tests/test_oracle_vs_hf.py).  Tolerance as tests/test_train_gpu.py."""
    from magma_amd.config import MultimodalConfig
    from magma_amd.language_model import GPTJConfig
    from magma_amd.magma import Magma
    from magma_amd.train_engine import MagmaEngine
    from oracle.model import (OracleConfig, ViTConfig, build_labels, init_params, init_vit_params, lm_forward,
                              pooled_prefix_fwd, vit_encoder_fwd)
    import torch.nn.functional as F
    s_img, d = 4, 512
    mcfg = MultimodalConfig(batch_size=2, train_steps=1, encoder_name="clip", image_seq_len=s_img, image_size=224,
                            freeze_img_encoder=False, use_image_embed_layernorm=True, image_embed_dropout_prob=0.1,
                            adapter_config={"mlp": {"adapter_type": "normal", "downsample_factor": 4}},
                            image_enc_lr=2.0e-6, lr_decay_iters=1000)
    lm_cfg = GPTJConfig(vocab_size=1056, hidden_size=d, num_layers=2, num_heads=2, rotary_dim=64, intermediate_size=2048,
                        max_position_embeddings=128)
    model = Magma(mcfg, device=dev, lm_config=lm_cfg)
    cfg = OracleConfig.tiny(n_positions=128)
    v = ViTConfig()
    params = {k: t for k, t in init_params(cfg, seed=31).items() if not k.startswith("image_prefix.")}
    for k in params:
        if ".adapter." in k:
            params[k] = params[k] * 20
    params.update(init_vit_params(v, seed=5))
    g = torch.Generator().manual_seed(9)
    params["image_prefix.proj.weight"] = torch.randn(s_img * d, v.out_dim, generator=g) * v.out_dim ** -0.5
    params["image_prefix.proj.bias"] = torch.randn(s_img * d, generator=g) * 0.02
    params["image_prefix.ln.weight"] = 1.0 + torch.randn(d, generator=g) * 0.05
    params["image_prefix.ln.bias"] = torch.randn(d, generator=g) * 0.02
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing, unexpected)
    model.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(model)
    eng.train()
    B, S = 2, model.seq_len
    images = torch.randn(B, 3, 224, 224, generator=g).to(torch.bfloat16).float()
    caps = torch.full((B, S), cfg.eos_token, dtype=torch.int64)
    caps[0, :23] = torch.randint(0, 1000, (23,), generator=g)
    caps[1, :11] = torch.randint(0, 1000, (11,), generator=g)
    mask = (torch.rand(B, s_img, d, generator=g) < 0.9).float() / 0.9
    names = [k for k in params if ".adapter." in k or k.startswith("image_prefix.")]

    def oracle(dtype):
        p = {k: (t.detach().to(dtype).clone() if t.is_floating_point() else t) for k, t in params.items()}
        for k in names:
            p[k].requires_grad_(True)
        prefix = pooled_prefix_fwd(p, d, s_img, vit_encoder_fwd(p, v, images.to(dtype)), dropout_mask=mask.to(dtype))
        labels = build_labels(s_img, caps, cfg.eos_token)
        words = F.embedding(caps, p["lm.transformer.wte.weight"]).to(prefix.dtype)
        out = lm_forward(p, cfg, inputs_embeds=torch.cat((prefix, words[:, : S - s_img, :]), dim=1), labels=labels)
        out["loss"].backward()
        return float(out["loss"].detach()), {k: p[k].grad.float() for k in names}

    loss_ref, g_ref = oracle(torch.float32)
    loss_bf, g_bf = oracle(torch.bfloat16)
    out = eng(images.to(dev), caps.to(dev), dropout_mask=mask.to(dev))
    assert abs(float(out.loss) - loss_ref) <= 2 * abs(loss_bf - loss_ref) + 3e-3 * abs(loss_ref), (float(out.loss), loss_ref, loss_bf)
    eng.backward(out.loss)
    name_of = {id(p): n for n, p in model.named_parameters()}
    seen, bad = set(), []
    dots = n1 = n2 = bd = b1 = 0.0
    thirds = 0
    for grp in eng.groups:
        for p in grp.params:
            n = name_of[id(p)]
            n = "lm." + n if n.startswith("transformer.") else n
            if n in seen or n not in g_ref:
                continue
            seen.add(n)
            got, ref, gb = eng.grad_of(p).float().cpu().reshape(-1), g_ref[n].reshape(-1), g_bf[n].reshape(-1)
            e_hip, e_bf = rel(got, ref), rel(gb, ref)
            if e_hip > 2 * e_bf + 3e-2:
                bad.append((n, e_hip, e_bf))
            if n.endswith(("attn.in_proj_weight", "attn.in_proj_bias")):
                # the q, k and v rows each on their own: in the whole tensor the K rows (the gradient mg_attn_small_bwd_bf16
                # writes as dk) are diluted by the V rows, and a few per cent of error in them stay under the floor.  (The k third
                # of the BIAS is zero in exact arithmetic -- a constant added to every key's score leaves the softmax as it is --
                # so its reference is the fp32 oracle's roundoff, ~1e-9, and the rule compares two such residues there.)
                for third, (a, r, b) in zip("qkv", zip(got.chunk(3), ref.chunk(3), gb.chunk(3))):
                    thirds += 1
                    t_hip, t_bf = rel(a, r), rel(b, r)
                    print(f"[thirds] {n} {third} rows: rel {t_hip:.3e}, bf16 oracle {t_bf:.3e}, |ref| {float(r.norm()):.3e}")
                    if t_hip > 2 * t_bf + 3e-2:
                        bad.append((f"{n}, {third} rows", t_hip, t_bf))
            dots += float((got * ref).sum()); n1 += float((got * got).sum()); n2 += float((ref * ref).sum())
            bd += float((gb * ref).sum()); b1 += float((gb * gb).sum())
    assert len(seen) == len(g_ref) and len(seen) > 150, (len(seen), len(g_ref), sorted(set(g_ref) - seen)[:5])
    assert thirds == 72, thirds                 # 12 blocks x (weight, bias) x (q, k, v)
    assert not bad, bad[:8]
    cos_hip, cos_bf = dots / (n1 ** 0.5 * n2 ** 0.5), bd / (b1 ** 0.5 * n2 ** 0.5)
    assert 1 - cos_hip <= 2 * (1 - cos_bf) + 1e-3, (cos_hip, cos_bf)
    eng.step()
    eng.eval()
    assert torch.isfinite(eng(images.to(dev), caps.to(dev)).loss)


def test_attn_small_backward(dev):
    """mg_attn_small_bwd_bf16 against autograd through fp32 softmax attention (non-causal, head dim 64)."""
    from magma_amd import ops
    for (B, S, H) in [(2, 50, 12), (1, 7, 2), (3, 64, 1)]:
        g = torch.Generator(device=dev).manual_seed(S)
        qkv = (torch.randn(B * S, 3 * H * 64, device=dev, generator=g) * 0.7).to(torch.bfloat16)
        do = torch.randn(B * S, H * 64, device=dev, generator=g).to(torch.bfloat16)
        x = qkv.float().requires_grad_(True)
        q, k, vv = (u.reshape(B, S, H, 64).permute(0, 2, 1, 3) for u in x.chunk(3, dim=-1))
        o = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ vv).permute(0, 2, 1, 3).reshape(B * S, H * 64)
        o.backward(do.float())
        got = ops.attn_small_bwd(qkv, do, B, S, H)
        assert rel(got, x.grad) < 1e-2, (B, S, H, rel(got, x.grad))


def test_magma_with_clip_vit_encoder(dev):
    """Magma built from a config that selects encoder_name "clip": embed() yields image_seq_len prefix tokens per image."""
    from magma_amd.config import MultimodalConfig
    from magma_amd.language_model import GPTJConfig
    from magma_amd.magma import Magma
    cfg = MultimodalConfig(batch_size=2, train_steps=1, encoder_name="clip", image_seq_len=4, image_size=224,
                           adapter_config={"mlp": {"adapter_type": "normal", "downsample_factor": 4}})
    lm_cfg = GPTJConfig(vocab_size=1056, hidden_size=512, num_layers=2, num_heads=2, rotary_dim=64, intermediate_size=2048,
                        max_position_embeddings=256)
    model = Magma(cfg, device=dev, lm_config=lm_cfg)
    model.eval()
    assert model.image_prefix.pooled and model.image_prefix_seq_len == 4
    emb = model.embed([torch.randn(2, 3, 224, 224), torch.randint(0, 1000, (2, 5))])
    assert emb.shape == (2, 4 + 5, 512) and bool(torch.isfinite(emb.float()).all())
    toks = model.generate(emb, max_steps=3, temperature=0.0, decode=False, stop_on_eos=False)
    assert toks.shape == (2, 9 + 3)


# ----------------------------------------------------------------------------------------------------------------------------
# Adapter options of the reference (magma/adapters.py:11-24): ``activation`` and ``add_layernorm``
# ----------------------------------------------------------------------------------------------------------------------------
import functools  # noqa: E402

_ACTS = {"relu": torch.nn.ReLU, "gelu": torch.nn.GELU, "gelu_tanh": functools.partial(torch.nn.GELU, approximate="tanh")}
OPTION_CASES = [("normal", None, "gelu", True), ("normal", "normal", "relu", True), ("parallel", "scaled_parallel", "gelu_tanh", True),
                ("normal", None, "gelu_tanh", False)]


def _build_opts(dev, mlp_type, attn_type, act, ln):
    from magma_amd.config import MultimodalConfig
    from magma_amd.image_encoders import ModifiedResNetTrunk
    from magma_amd.language_model import GPTJConfig
    from magma_amd.magma import Magma
    extra = dict(add_layernorm=ln, activation=_ACTS[act])
    ad = {"mlp": dict(adapter_type=mlp_type, downsample_factor=4, **extra)}
    if attn_type:
        ad["attention"] = dict(adapter_type=attn_type, downsample_factor=8, **extra)
    cfg = MultimodalConfig(batch_size=2, train_steps=1, encoder_name="clip_resnet_large", adapter_config=ad, image_size=64,
                           freeze_img_encoder=False, use_image_embed_layernorm=True, image_embed_dropout_prob=0.1)
    lm_cfg = GPTJConfig(vocab_size=1056, hidden_size=512, num_layers=2, num_heads=2, rotary_dim=64, intermediate_size=2048,
                        max_position_embeddings=256)
    enc = ModifiedResNetTrunk((1, 1, 2, 1), 16, 64, device=dev, dtype=torch.bfloat16)
    return Magma(cfg, device=dev, lm_config=lm_cfg, enc=enc)


def _opt_params(mlp_type, attn_type, act, ln, seed):
    from oracle.model import OracleConfig, init_params
    cfg = OracleConfig.tiny(mlp_adapter_hidden=128, attn_adapter_hidden=64 if attn_type else 0, mlp_adapter_type=mlp_type,
                            attn_adapter_type=attn_type or "normal", adapter_act=act, adapter_layernorm=ln)
    p = init_params(cfg, seed=seed)
    lin = ("1.", "3.") if ln else ("0.", "2.")
    for k in p:        # larger projections than the 1e-3 init so that the adapter arithmetic is visible; the LayerNorm stays O(1)
        if ".adapter." in k and k.split(".adapter.")[1].startswith(lin):
            p[k] = p[k] * 20
    return cfg, p


@pytest.mark.parametrize("mlp_type,attn_type,act,ln", OPTION_CASES)
def test_adapter_options_inference_vs_oracle(dev, mlp_type, attn_type, act, ln):
    """Prefill, cached steps (whatever launch structure the option set allows: the folded / grouped blocks for plain ReLU adapters
    with another activation code, the generic block with an extra LayerNorm launch otherwise) and the full-sequence forward."""
    from oracle.model import generate_greedy, lm_forward
    cfg, p = _opt_params(mlp_type, attn_type, act, ln, seed=7)
    model = _build_opts(dev, mlp_type, attn_type, act, ln)
    missing, unexpected = model.load_checkpoint_state(p)
    assert not unexpected and not missing, (missing, unexpected)
    model.eval()
    lm = {k: v for k, v in p.items() if k.startswith("lm.")}
    lmb = bf16_params(lm)
    g = torch.Generator().manual_seed(2)
    emb = torch.randn(2, 10, cfg.d_model, generator=g).to(torch.bfloat16).float()
    steps = 4
    with torch.no_grad():
        ref_toks, ref_logits = generate_greedy(lm, cfg, emb, steps, stop_on_eos=False)
        _, bf_logits = generate_greedy(lmb, cfg, emb.to(torch.bfloat16), steps, stop_on_eos=False)
        # the option must matter: the same weights under the default activation give other logits
        import dataclasses
        other = dataclasses.replace(cfg, adapter_act="relu" if act != "relu" else "gelu")
        assert rel(lm_forward(lm, other, inputs_embeds=emb)["logits"], lm_forward(lm, cfg, inputs_embeds=emb)["logits"]) > 5e-3
        out = model.lm(inputs_embeds=emb.to(torch.bfloat16).cuda(), use_cache=True, cache_hint=steps)
        assert rel(out.logits[:, -1], ref_logits[0]) <= 2 * rel(bf_logits[0], ref_logits[0]) + 2e-3
        cache, S0 = out.past_key_values, emb.shape[1]
        for i in range(1, steps):
            o = model.lm(input_ids=ref_toks[:, S0 + i - 1: S0 + i].cuda(), use_cache=True, past_key_values=cache)
            assert rel(o.logits[:, -1], ref_logits[i]) <= 2 * max(rel(bf_logits[i], ref_logits[i]), 5e-3) + 2e-3, i
        full = model.lm(inputs_embeds=emb.to(torch.bfloat16).cuda())
        assert rel(full.logits, lm_forward(lm, cfg, inputs_embeds=emb)["logits"]) < 2e-2


@pytest.mark.parametrize("mlp_type,attn_type,act,ln", OPTION_CASES[:3])
def test_adapter_options_train_gradients(dev, mlp_type, attn_type, act, ln):
    """Gradients of every trainable tensor -- the adapters' LayerNorm gains / biases included -- against autograd through the oracle.
    Per tensor: err(HIP) <= 2 x err(bf16 autograd) + 3e-2; a tensor whose bf16-autograd error is itself above 10 % (small BatchNorm
    gains deep in the trunk: rounding noise, not signal) is held to 3 x that error instead; adapter tensors always to the first
    rule; all tensors together: 1 - cosine no larger than twice the bf16 autograd's + 1e-3."""
    from magma_amd.train_engine import MagmaEngine
    from oracle.model import magma_forward
    cfg, params = _opt_params(mlp_type, attn_type, act, ln, seed=29)
    model = _build_opts(dev, mlp_type, attn_type, act, ln)
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing, unexpected)
    model.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(model)
    eng.train()
    g = torch.Generator().manual_seed(3)
    B, S = 2, model.seq_len
    images = torch.randn(B, 3, 64, 64, generator=g)
    caps = torch.full((B, S), cfg.eos_token, dtype=torch.int64)
    caps[0, :23] = torch.randint(0, 1000, (23,), generator=g)
    caps[1, :11] = torch.randint(0, 1000, (11,), generator=g)
    mask = (torch.rand(B, 4, cfg.d_model, generator=g) < 0.9).float() / 0.9

    def oracle_grads(dtype):
        p = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v) for k, v in params.items()}
        names = [k for k in p if (".adapter." in k or "adapter_scale" in k or k.startswith("image_prefix.")) and "running_" not in k]
        for k in names:
            p[k].requires_grad_(True)
        out = magma_forward(p, cfg, images.to(dtype), caps, dropout_mask=mask.to(dtype))
        out["loss"].backward()
        return float(out["loss"]), {k: p[k].grad.float() for k in names}

    loss_ref, g_ref = oracle_grads(torch.float32)
    loss_bf, g_bf = oracle_grads(torch.bfloat16)
    out = eng(images.to(dev), caps.to(dev), dropout_mask=mask.to(dev))
    assert abs(float(out.loss) - loss_ref) <= 2 * abs(loss_bf - loss_ref) + 3e-3 * abs(loss_ref)
    eng.backward(out.loss)
    name_of = {id(p): n for n, p in model.named_parameters()}
    dots = n1 = n2 = bd = b1 = 0.0
    seen, bad = set(), []
    for grp in eng.groups:
        for p in grp.params:
            n = name_of[id(p)]
            n = "lm." + n if n.startswith("transformer.") else n
            if n in seen or n not in g_ref:
                continue
            seen.add(n)
            got, ref = eng.grad_of(p).float().cpu().reshape(-1), g_ref[n].reshape(-1)
            e_hip, e_bf = rel(got, ref), rel(g_bf[n].reshape(-1), ref)
            noisy = e_bf >= 0.1 and ".adapter." not in n
            if "adapter_scale" not in n and e_hip > (3 * e_bf if noisy else 2 * e_bf + 3e-2):
                bad.append((n, e_hip, e_bf))
            dots += float((got * ref).sum()); n1 += float((got * got).sum()); n2 += float((ref * ref).sum())
            gb = g_bf[n].reshape(-1)
            bd += float((gb * ref).sum()); b1 += float((gb * gb).sum())
    assert not bad, bad
    assert len(seen) == len(g_ref), set(g_ref) - seen
    assert any(".adapter.0.weight" in n and g_ref[n].ndim == 1 for n in seen) == ln      # the adapters' LayerNorm gains are trained
    cos_hip, cos_bf = dots / (n1 ** 0.5 * n2 ** 0.5), bd / (b1 ** 0.5 * n2 ** 0.5)
    print("cosine: hip", cos_hip, "bf16 autograd", cos_bf)
    assert 1 - cos_hip <= 2 * (1 - cos_bf) + 1e-3, (cos_hip, cos_bf)
    eng.step()
    eng.eval()
    assert torch.isfinite(eng(images.to(dev), caps.to(dev)).loss)
