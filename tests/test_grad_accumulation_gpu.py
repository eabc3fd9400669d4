"""Gradient accumulation: a window of N micro-steps leaves, in every gradient buffer, the sum of what its micro-batches give alone.

configs/MAGMA_v1.yml trains with gradient_accumulation_steps: 8 and every other numeric training test runs windows of one, where
``=`` and ``+=`` into a zeroed buffer give the same bits.  Here every engine is built with gradient_accumulation_steps = 3 (three
tell "keeps only the last" from "keeps the last two") and three micro-batches that differ where it matters: images, dropout masks,
token ids, label counts, and caption lengths that make the truncated sequence 64, 128 and 64 positions long, so that every
cached workspace is re-sized inside the window.

Protocol of a case (``run_window_case``):
  parts     for i in 0..2: zero every flat gradient, micro_steps = 0, forward, backward, clone -> g_i; all of it once more -> g_i'
  window    zero, micro_steps = 0; forward / backward / step() three times as train_loop.train_step does; the gradients are
            cloned after the third backward.  step() number 1 and 2 must leave masters, m, v, the bf16 copies, the gradient
            buffers, global_steps and the learning rates bit-identical
  assert    per trainable tensor (named_parameters, so a failure names it):  |G - sum_i g_i| <= kernel_compare.accumulation_bound
            = 8 u32 sum|g_i| + 4 sum|g_i - g_i'| + 1e-5 rms(sum g_i), after the two conditions that do not look at the window:
            the second run of the parts meets the bound against the first, and every part is >= 100 bounds large somewhere in
            every tensor (only a part that is identically zero in both runs is excused; the names are printed, and none of them
            may be a weight, bias, gain or normalisation affine).

Every tensor of a case is compared before the case fails, so one run shows all the offenders."""
import pytest
import torch

import kernel_compare as kc
from accumulation_common import N, flat_grads, forward_backward, micro_batches, take_parts, zero_window

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-20))


# ---------------------------------------------------------------------------------------------------------------------------
# the protocol
# ---------------------------------------------------------------------------------------------------------------------------
def state_of(eng):
    return ([t.clone() for grp in eng.groups for t in (grp.master, grp.m, grp.v, grp.grad, grp.model)],
            eng.global_steps, list(eng.lr_scheduler.get_lr()), eng.lr_scheduler.last_step)


def assert_same_state(a, b, what):
    assert a[1:] == b[1:], (what, a[1:], b[1:])
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), f"{what}: {('master', 'm', 'v', 'grad', 'bf16 copy')[i % 5]} of group {i // 5} changed"


def run_window(eng, batches):
    """Exactly train_loop.train_step's sequence -> the flat gradients after the third backward, BEFORE the third step()."""
    zero_window(eng)
    for i in range(N):
        forward_backward(eng, batches, i)
        assert eng.micro_steps == i + 1
        if i == N - 1:
            return flat_grads(eng)
        before = state_of(eng)
        eng.step()
        assert_same_state(before, state_of(eng), f"step() on micro-step {i + 1} of {N}")


def trainable(eng):
    seen, out = set(), []
    for n, p in eng.module.named_parameters():
        if eng.is_trainable(p) and id(p) not in seen:
            seen.add(id(p))
            out.append((n, p))
    assert sum(len(g.params) for g in eng.groups) == len(out)
    return out


def view(eng, flats, p):
    gi, _ = eng._where[id(p)]
    return eng.groups[gi].view(flats[gi], p)


def compare_window(eng, G, parts, repeats, label):
    """Every trainable tensor of the window against its parts -> (worst ratio, worst reference-against-reference ratio)."""
    fails, excused, worst, worst_self = [], [], (0.0, ""), (0.0, "")
    for n, p in trainable(eng):
        try:
            r = kc.assert_accumulation(view(eng, G, p), [view(eng, f, p) for f in parts], [view(eng, f, p) for f in repeats],
                                       f"{label} {n} {tuple(p.shape)}")
        except AssertionError as e:
            fails.append(str(e))
            continue
        worst, worst_self = max(worst, (r["worst"], n)), max(worst_self, (r["self"], n))
        if r["zero_parts"]:
            excused.append((n, r["zero_parts"]))
    print(f"[accumulation] {label}: {len(trainable(eng))} tensors, worst window err/bound {worst[0]:.3g} ({worst[1]}), worst "
          f"reference-against-reference {worst_self[0]:.3g} ({worst_self[1]}); identically-zero parts excused: {excused or 'none'}")
    for n, _ in excused:
        assert not n.endswith(("weight", "bias", "gain")), f"{label}: {n} has an identically zero part: choose other inputs"
    assert not fails, f"{label}: {len(fails)} tensor(s) fail:\n" + "\n".join(fails[:12])
    return worst[0], worst_self[0]


def finish_window(eng):
    """The window's third step(): the one that applies the update, zeroes the buffers and advances the schedule."""
    steps, sched = eng.global_steps, eng.lr_scheduler.last_step
    eng.step()
    assert eng.global_steps == steps + 1 and eng.micro_steps == N and eng.lr_scheduler.last_step == sched + 1
    assert all(float(g.grad.abs().sum()) == 0.0 for g in eng.groups)


def run_window_case(eng, batches, label, third_step=True):
    """parts, repeats, window, comparison, third step().  -> (G, parts, repeats); with third_step=False the engine is left
    right before the window's third step() (the base case checks that step per element)."""
    assert eng.gas == N
    parts = take_parts(eng, batches)
    repeats = take_parts(eng, batches)
    G = run_window(eng, batches)
    compare_window(eng, G, parts, repeats, label)
    if third_step:
        finish_window(eng)
    return G, parts, repeats


# ---------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------
def amplified(params, linear_only=None):
    for k in params:
        if ".adapter." in k and (linear_only is None or k.split(".adapter.")[1].startswith(linear_only)):
            params[k] = params[k] * 20
    return params


def reduced_engine(dev, oracle_kw=None, seed=21, freeze_lm=True, linear_only=None, prepare=None, res=64, **build_kw):
    """build_reduced_magma at n_positions = 128 with oracle-initialised weights (adapter projections x 20, as
    test_gradients_and_step has them), gradient_accumulation_steps = 3, truncating engine."""
    from magma_amd.testing import build_reduced_magma
    from magma_amd.train_engine import MagmaEngine
    from oracle.model import OracleConfig, init_params
    cfg = OracleConfig.tiny(n_positions=128, **(oracle_kw or {}))
    params = amplified(init_params(cfg, seed=seed), linear_only)
    model = build_reduced_magma(dev, n_positions=128, min_lr=1e-4, weight_decay=0.05, resolution=res, image_size=res, **build_kw)
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing, unexpected)
    if not freeze_lm:
        model.config.freeze_lm = False
        for p in model.lm.parameters():
            p.requires_grad = True
    model.config.gradient_accumulation_steps = N
    eng = MagmaEngine(model, truncate=True)
    if prepare is not None:
        prepare(eng)
    eng.train()
    return cfg, params, model, eng, micro_batches(seed + 100, cfg.eos_token, model.seq_len, (res // 32) ** 2, cfg.d_model, res=res)


# ---------------------------------------------------------------------------------------------------------------------------
# 1 / 2: the base model, with the extra checks of the first window's step and a second window
# ---------------------------------------------------------------------------------------------------------------------------
def check_step(eng, G, label):
    """The window's third step(): AdamW per element from g = G, the norm of G and grad_scale = 1 / N; counters; buffers."""
    step = eng.global_steps + 1
    lrs = eng.lr_scheduler.get_lr()
    sched_before = eng.lr_scheduler.last_step
    before = [(g.master.clone(), g.m.clone(), g.v.clone()) for g in eng.groups]
    norm_sq = sum(kc.f64(g).pow(2).sum() for g in G)
    eng.step()
    assert eng.global_steps == step and eng.micro_steps == N and eng.lr_scheduler.last_step == sched_before + 1
    assert eng.grad_norm() == pytest.approx(float(norm_sq.sqrt()) / N, rel=1e-4)
    print(f"[accumulation] {label} step {step}: |G| / {N} = {float(norm_sq.sqrt()) / N:.4g} against the clip threshold {eng.clip:g}")
    for g, gr, (p0, m0, v0), lr in zip(eng.groups, G, before, lrs):
        assert lr > 0
        R = kc.adamw_reference(p0, m0, v0, gr, norm_sq, lr, eng.betas[0], eng.betas[1], eng.eps, g.wd, step, eng.clip, 1.0 / N)
        for name, got in (("m", g.m), ("v", g.v), ("p", g.master), ("p_bf16", g.model)):
            kc.assert_elementwise(got, *R[name], f"{label} step {step}, group lr_max={g.lr_max:g}: {name}")
        assert float(g.grad.abs().sum()) == 0.0


def oracle_window(cfg, params, batches):
    """Mean of the three micro-batches' oracle gradients, fp32 and bf16 (the oracle knows nothing of windows)."""
    from test_train_gpu import oracle_grads
    mean = {}
    for dtype in (torch.float32, torch.bfloat16):
        acc = None
        for images, caps, mask in batches:
            _, g = oracle_grads(cfg, params, images, caps, mask, dtype)
            acc = g if acc is None else {k: acc[k] + g[k] for k in g}
        mean[dtype] = {k: v / N for k, v in acc.items()}
    return mean[torch.float32], mean[torch.bfloat16]


def base_case(dev, label, with_oracle):
    cfg, params, model, eng, batches = reduced_engine(dev, dict(mlp_adapter_hidden=128, attn_adapter_hidden=0), mlp_factor=4)
    G, parts, _ = run_window_case(eng, batches, label + " window 1", third_step=False)
    if with_oracle:
        g_ref, g_bf = oracle_window(cfg, params, batches)
        dots = n1 = n2 = 0.0
        seen = set()
        for n, p in trainable(eng):
            k = "lm." + n if n.startswith("transformer.") else n
            assert k in g_ref, k
            seen.add(k)
            got, ref = view(eng, G, p).float().cpu() / N, g_ref[k]
            e_hip, e_bf = rel(got, ref), rel(g_bf[k], ref)
            assert e_hip <= 2 * e_bf + 3e-2, f"{k}: window / {N} against the oracle mean: {e_hip:.3e} vs bf16-autograd {e_bf:.3e}"
            dots += float((got * ref).sum()); n1 += float((got * got).sum()); n2 += float((ref * ref).sum())
        assert len(seen) == len(g_ref), set(g_ref) - seen
        cos = dots / (n1 ** 0.5 * n2 ** 0.5)
        print(f"[accumulation] {label}: window / {N} against the oracle mean, cosine {cos:.6f}")
        assert cos > 0.999, cos
    masters = [g.master.clone() for g in eng.groups]
    check_step(eng, G, label)
    assert all(not torch.equal(a, g.master) for a, g in zip(masters, eng.groups)), "the first step moved nothing: window 2 tests nothing new"
    # a second window straight after the step: parts at the NEW weights.  A buffer that kept something, a packed weight copy
    # that was not refreshed, or a workspace of the first window's last shape shows here
    G2, parts2, _ = run_window_case(eng, batches, label + " window 2", third_step=False)
    assert not any(torch.equal(a[i], b[i]) for a, b in zip(parts, parts2) for i in range(len(a))), "the parts did not see the new weights"
    check_step(eng, G2, label)
    assert eng.global_steps == 2


def test_base_window_against_parts_oracle_and_adamw(dev):
    """v1 adapters, trainable CLIP trunk on frozen BatchNorm statistics, every switch at its default."""
    base_case(dev, "base", with_oracle=True)


def test_base_with_the_ab_switches_off(dev, monkeypatch):
    """The fp32 temporary + scale_rows_acc weight-gradient path, the two-pass bn_param_grad path and one re-layout per
    convolution: the forms the A/B switches keep alive."""
    from magma_amd import train_engine
    for sw in ("_WGRAD_INPLACE", "_BN_GRAD_FUSED", "_CONV_PLAN"):
        monkeypatch.setattr(train_engine, sw, False)
    base_case(dev, "switches off", with_oracle=False)


# ---------------------------------------------------------------------------------------------------------------------------
# 3: BatchNorm on batch statistics
# ---------------------------------------------------------------------------------------------------------------------------
def batch_statistics_case(dev, res):
    def prepare(eng):
        eng.train(bn_batch_stats=True)

    _, _, model, eng, batches = reduced_engine(dev, dict(mlp_adapter_hidden=128, attn_adapter_hidden=0), seed=31, mlp_factor=4,
                                               prepare=prepare, res=res)
    bns = [m for m in model.image_prefix.enc.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for bn in bns:
        eng._bn_vectors(bn)                       # the engine's own lazy fp32 copies of the running statistics
    start = {k: (a.clone(), b.clone()) for k, (a, b) in eng._bn_stats.items()}
    assert len(start) == len(bns) > 10

    def stats_then_restore():
        now = {k: (a.clone(), b.clone()) for k, (a, b) in eng._bn_stats.items()}
        for k, (a, b) in start.items():
            eng._bn_stats[k][0].copy_(a); eng._bn_stats[k][1].copy_(b)
        return now

    label = f"batch statistics {res}x{res}"
    parts = take_parts(eng, batches)
    after_parts = stats_then_restore()
    repeats = take_parts(eng, batches)
    after_repeats = stats_then_restore()
    for n, p in trainable(eng):
        if n.startswith("image_prefix.enc."):
            for i in range(N):
                assert torch.equal(view(eng, parts[i], p), view(eng, repeats[i], p)), f"{label}: {n}, micro-batch {i}: two runs differ"
    G = run_window(eng, batches)
    compare_window(eng, G, parts, repeats, label)
    finish_window(eng)
    worst = 0.0
    for bn in bns:
        k = id(bn)
        for j, what in enumerate(("running_mean", "running_var")):
            a, w = after_parts[k][j], eng._bn_stats[k][j]
            assert not torch.equal(a, start[k][j]), "the statistics did not move"
            bound = kc.accumulation_bound([a], [after_repeats[k][j]])
            worst = max(worst, kc.assert_elementwise(w, kc.f64(a), bound, f"{label} {what} of {a.numel()} channels"))
    print(f"[accumulation] {label}: running statistics after the window against after the parts, worst err/bound {worst:.3g}")


@pytest.mark.parametrize("res", [64, 32])
def test_batch_statistics_batchnorm_window(dev, res):
    """train(bn_batch_stats=True): gradients as in every other case; the running statistics after the window equal those after
    the parts pass (the same three updates in the same order) under the same bound.  The running statistics are snapshotted
    before the parts and restored before the repeat and before the window.

    At 64 x 64 the three stem units have 2048 rows per channel, eight partial sums of 256 rows each; at 32 x 32 no unit has more
    than two.  This case found that the mode was not reproducible: its per-channel sums (forward statistics, backward dbeta /
    dgamma) were fp32 atomics, three or more of which do not commute; the sums feed a bf16 rounding (bn_apply, bn_bwd_dz), and in
    about 3 % of the forwards of the first micro-batch one rounding in the stem fell the other way, after which layer4's
    BatchNorm over 8 rows per channel turned that last-place difference into another loss (6.99626 instead of 6.99704) and
    gradients 3 .. 26 % away in 72 of the 78 tensors.  The sums now come from ops.colsum(deterministic=True), partials added in
    row order, and the trunk's gradients in this mode are the same bits in every run, which is asserted here for every trunk
    tensor and micro-batch before the window is looked at."""
    batch_statistics_case(dev, res)


# ---------------------------------------------------------------------------------------------------------------------------
# 4: adapter variants
# ---------------------------------------------------------------------------------------------------------------------------
def test_v2_adapters_window(dev):
    _, _, _, eng, batches = reduced_engine(dev, dict(mlp_adapter_hidden=64, attn_adapter_hidden=64), mlp_factor=8, attn_factor=8)
    run_window_case(eng, batches, "v2")


def test_scaled_parallel_adapters_window(dev):
    """_par_adapter_backward: the scalar ds into adapter_scale, the .add_ of gb, scale_rows_acc into W_up."""
    ad = {"mlp": {"adapter_type": "scaled_parallel", "downsample_factor": 4},
          "attention": {"adapter_type": "scaled_parallel", "downsample_factor": 8}}
    okw = dict(mlp_adapter_hidden=128, attn_adapter_hidden=64, mlp_adapter_type="scaled_parallel", attn_adapter_type="scaled_parallel")
    _, _, model, eng, batches = reduced_engine(dev, okw, seed=23, adapter_config=ad)
    names = [n for n, _ in trainable(eng)]
    assert any("adapter_scale" in n for n in names), names
    run_window_case(eng, batches, "scaled_parallel")


def test_layernorm_gelu_adapter_window(dev):
    """An adapter with its own LayerNorm and nn.GELU: the erf pass, the LayerNorm backward's gain / bias sums."""
    ad = {"mlp": dict(adapter_type="normal", downsample_factor=4, add_layernorm=True, activation=torch.nn.GELU)}
    okw = dict(mlp_adapter_hidden=128, attn_adapter_hidden=0, adapter_act="gelu", adapter_layernorm=True)
    _, _, model, eng, batches = reduced_engine(dev, okw, seed=29, linear_only=("1.", "3."), adapter_config=ad)
    assert any(n.endswith(".adapter.0.weight") and p.ndim == 1 for n, p in trainable(eng))
    run_window_case(eng, batches, "LayerNorm + GELU adapter")


# ---------------------------------------------------------------------------------------------------------------------------
# 5 / 6: the whole language model trainable; per-block recompute
# ---------------------------------------------------------------------------------------------------------------------------
def test_freeze_lm_false_window(dev):
    """index_add_ into wte, the lm_head bias through cs[:V], ln_f, every block's LayerNorm and Linear tensors."""
    _, _, model, eng, batches = reduced_engine(dev, seed=27, freeze_lm=False)
    names = [n for n, _ in trainable(eng)]
    for piece in ("wte.weight", "lm_head.weight", "lm_head.bias", "ln_f.weight", "q_proj.weight", "out_proj.weight", "ln_1.bias"):
        assert any(piece in n for n in names), (piece, names[:20])
    run_window_case(eng, batches, "freeze_lm false")


def test_recompute_window(dev):
    def prepare(eng):
        eng.recompute = True
    _, _, _, eng, batches = reduced_engine(dev, dict(mlp_adapter_hidden=128, attn_adapter_hidden=0), mlp_factor=4, prepare=prepare)
    run_window_case(eng, batches, "recompute")
    assert eng.recompute


# ---------------------------------------------------------------------------------------------------------------------------
# 7: the other encoders
# ---------------------------------------------------------------------------------------------------------------------------
def pooled_engine(dev, encoder_name, s_img, res, enc_params, enc_out_dim):
    from magma_amd.config import MultimodalConfig
    from magma_amd.language_model import GPTJConfig
    from magma_amd.magma import Magma
    from magma_amd.train_engine import MagmaEngine
    from oracle.model import OracleConfig, init_params
    d = 512
    mcfg = MultimodalConfig(batch_size=2, train_steps=1, encoder_name=encoder_name, image_seq_len=s_img, image_size=res,
                            freeze_img_encoder=False, use_image_embed_layernorm=True, image_embed_dropout_prob=0.1,
                            adapter_config={"mlp": {"adapter_type": "normal", "downsample_factor": 4}},
                            image_enc_lr=2.0e-6, lr_decay_iters=1000)
    lm_cfg = GPTJConfig(vocab_size=1056, hidden_size=d, num_layers=2, num_heads=2, rotary_dim=64, intermediate_size=2048,
                        max_position_embeddings=128)
    model = Magma(mcfg, device=dev, lm_config=lm_cfg)
    cfg = OracleConfig.tiny(n_positions=128)
    params = amplified({k: t for k, t in init_params(cfg, seed=31).items() if not k.startswith("image_prefix.")})
    params.update(enc_params)
    g = torch.Generator().manual_seed(9)
    params["image_prefix.proj.weight"] = torch.randn(s_img * d, enc_out_dim, generator=g) * enc_out_dim ** -0.5
    params["image_prefix.proj.bias"] = torch.randn(s_img * d, generator=g) * 0.02
    params["image_prefix.ln.weight"] = 1.0 + torch.randn(d, generator=g) * 0.05
    params["image_prefix.ln.bias"] = torch.randn(d, generator=g) * 0.02
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing[:4], unexpected[:4])
    model.config.gradient_accumulation_steps = N
    eng = MagmaEngine(model, truncate=True)
    eng.train()
    return eng, micro_batches(77, cfg.eos_token, model.seq_len, s_img, d, res=res)


def test_nfresnet50_window(dev):
    """NF-ResNet-50 unfrozen at the resolution of test_nfresnet50_train_gradients: weight_standardize_bwd's ``dw +=`` /
    ``dgain +=``, the bias_mult path."""
    from oracle.nfnet import NFResNetConfig, init_params
    eng, batches = pooled_engine(dev, "nfresnet50", 2, 128, init_params(NFResNetConfig(), seed=5), 2048)
    assert any(n.endswith(".gain") for n, _ in trainable(eng))
    run_window_case(eng, batches, "nfresnet50")


def test_clip_vit_window(dev):
    """CLIP ViT-B/32 with the pooled prefix: the class and positional embeddings' ``.add_``."""
    from oracle.model import ViTConfig, init_vit_params
    v = ViTConfig()
    eng, batches = pooled_engine(dev, "clip", 4, 224, init_vit_params(v, seed=5), v.out_dim)
    names = [n for n, _ in trainable(eng)]
    assert any("class_embedding" in n for n in names) and any("positional_embedding" in n for n in names)
    run_window_case(eng, batches, "clip vit")


# ---------------------------------------------------------------------------------------------------------------------------
# 8: fp8 training
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mx", ["1", "0"], ids=["mx", "row_scales"])
def test_fp8_training_window(dev, monkeypatch, mx):
    monkeypatch.setenv("MAGMA_TRAIN_FP8", "1")
    monkeypatch.setenv("MAGMA_TRAIN_FP8_MX", mx)
    _, _, _, eng, batches = reduced_engine(dev, dict(mlp_adapter_hidden=128, attn_adapter_hidden=0), seed=33, mlp_factor=4)
    assert eng.fp8 and eng.fp8_mx == (mx == "1")
    run_window_case(eng, batches, f"fp8 (MX {mx})")
    assert eng._fp8_packs, "fp8 mode did not pack any weight: the fp8 path was not taken"
