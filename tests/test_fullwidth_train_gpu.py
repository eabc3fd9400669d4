"""Training parity at BASELINE WIDTH and LENGTH (config[2] shapes: d 4096, 16 heads, ff 16384, V 50258, S = 2048, RN50x16 trunk at
224^2), one GPT-J block deep: loss and the gradient of every trainable tensor (MLP adapter, the whole CLIP trunk, prefix
projection + LayerNorm) from the explicit HIP backward against torch.autograd through the fp32 CPU oracle.

This is where the kernels of the measured training step run inside an oracle comparison: the 256x256 GEMM (M = 4096 rows,
N up to 16384, K up to 16384, GELU / GELU' / residual epilogues), flash attention forward and backward at S = 2048 with the
merged dqkv epilogue (inverse rotary), the rotary split that also emits q^T / k^T, the 50 258-column loss head on the target
rows -- the reduced-width tests (tests/test_train_gpu.py) never reach those variants.

Tolerance: per tensor  err(HIP bf16, oracle fp32) <= 2 x err(oracle autograd in bf16 on the CPU, oracle fp32)
+ 1e-2 rel-L2;  global cosine no further from 1 than twice the bf16 oracle's + 1e-3;  loss within 2 x the bf16 oracle's deviation + 3e-3 relative."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fullwidth_common as F  # noqa: E402

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.float().cpu().reshape(-1), b.float().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-20))


def test_gradients_full_width_s2048(dev):
    from magma_amd.testing import build_reduced_magma
    from magma_amd.train_engine import MagmaEngine
    from oracle.model import magma_forward
    cfg = F.full_width_config(n_positions=2048)
    params = F.full_width_params(cfg)
    model = build_reduced_magma(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=2048,
                                enc_width=96, enc_layers=(6, 8, 18, 8), resolution=224)
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing, unexpected)
    model.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(model)
    eng.train()
    B, S, P = 2, 2048, 49
    g = torch.Generator().manual_seed(7)
    images = torch.randn(B, 3, 224, 224, generator=g).to(torch.bfloat16).float()
    caps = torch.full((B, S), cfg.eos_token, dtype=torch.int64)
    caps[0, :61] = torch.randint(0, 50256, (61,), generator=g)
    caps[1, :17] = torch.randint(0, 50256, (17,), generator=g)
    mask = (torch.rand(B, P, cfg.d_model, generator=g) < 0.9).float() / 0.9
    names = [k for k in params if (".adapter." in k or k.startswith("image_prefix.")) and "running_" not in k]

    def oracle(dtype):
        p = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v) for k, v in params.items()}
        for k in names:
            p[k].requires_grad_(True)
        out = magma_forward(p, cfg, images.to(dtype), F.oracle_window(caps, P, cfg.eos_token), dropout_mask=mask.to(dtype))
        out["loss"].backward()
        return float(out["loss"].detach()), {k: p[k].grad.float() for k in names}

    loss_ref, g_ref = oracle(torch.float32)
    loss_bf, g_bf = oracle(torch.bfloat16)
    out = eng(images.to(dev), caps.to(dev), dropout_mask=mask.to(dev))
    assert abs(float(out.loss) - loss_ref) <= 2 * abs(loss_bf - loss_ref) + 3e-3 * abs(loss_ref), (float(out.loss), loss_ref, loss_bf)
    eng.backward(out.loss)
    name_of = {id(p): n for n, p in model.named_parameters()}
    seen, bad, worst = set(), [], []
    dots = n1 = n2 = bdots = bn1 = 0.0
    for grp in eng.groups:
        for p in grp.params:
            n = name_of[id(p)]
            n = "lm." + n if n.startswith("transformer.") else n
            if n in seen or n not in g_ref:
                continue
            seen.add(n)
            got, ref = eng.grad_of(p).float().cpu().reshape(-1), g_ref[n].reshape(-1)
            e_hip, e_bf = rel(got, ref), rel(g_bf[n], ref)
            worst.append((e_hip - 2 * e_bf, n, e_hip, e_bf))
            if e_hip > 2 * e_bf + 1e-2:
                bad.append((n, e_hip, e_bf))
            dots += float((got * ref).sum()); n1 += float((got * got).sum()); n2 += float((ref * ref).sum())
            gb = g_bf[n].reshape(-1)
            bdots += float((gb * ref).sum()); bn1 += float((gb * gb).sum())
    worst.sort(reverse=True)
    print("loss", float(out.loss), loss_ref, loss_bf, "| worst:", [(n, f"{a:.2e}", f"{b:.2e}") for _, n, a, b in worst[:5]],
          "| cos", dots / (n1 ** 0.5 * n2 ** 0.5), "| tensors", len(seen))
    assert len(seen) == len(g_ref) and len(seen) > 380, (len(seen), len(g_ref))
    assert not bad, bad[:8]
    cos_hip, cos_bf = dots / (n1 ** 0.5 * n2 ** 0.5), bdots / (bn1 ** 0.5 * n2 ** 0.5)
    print("cosine: hip", cos_hip, "bf16 oracle", cos_bf)
    assert 1 - cos_hip <= 2 * (1 - cos_bf) + 1e-3, (cos_hip, cos_bf)     # 0.999 at reduced width; relative here (S = 2048 sums)


def test_gradients_four_blocks_deep_full_width_s2048(dev):
    """Gradients AT DEPTH (reference train_loop.py:7-21 back-propagates through all blocks): four full-width GPT-J blocks
    (d 4096, ff 16384, V 50258), S = 2048, B = 1, a small trunk in front.  Every adapter / prefix / trunk gradient of the
    explicit HIP backward against torch.autograd through the fp32 CPU oracle -- the comparison that crosses block
    boundaries: the dgrad chain through the K-concatenated [W_out | W_up] forward, the attention output read at the wider
    row stride (ld_o), the merged attention-backward output (32-row-wave dK/dV + dQ kernels, inverse rotary in the
    epilogue) feeding the next block's residual gradient.  Criterion as in the one-block test for everything on the LM side
    (the adapters of all four blocks, prefix projection + LayerNorm): per tensor err(HIP) <= 2 x err(bf16 autograd on the
    CPU) + 1e-2 rel-L2, cosine no further from 1 than twice the bf16 oracle's.  The 4-token trunk in front (B = 1, 64 x 64
    pixels; it is only the sink of the gradient here -- its own parity at the real geometry is the one-block test above) gets
    2.5 x: measured (MI355X, round 5, identical with the round-4 attention-backward kernels) three BatchNorm gains of its first
    layers sit at 2.3-2.4 x the bf16 oracle's error (0.089-0.142 against 0.040-0.059), every other tensor below 2 x;
    worst adapter tensor per block 6.4 / 7.2 / 7.4 / 6.8 %.
    Measured again after the BatchNorm gain gradient was moved from the rounded unit output to the convolution output
    (ops.scale_rows_acc_bn_grad): layer2.0.bn2.weight 0.146 against 0.059 (2.46 x), bn1.weight 0.097 against 0.045 (2.17 x),
    layer2.0.bn1.weight 0.083 against 0.040 (2.11 x), bn1.bias 0.073 against 0.040 (1.84 x): the 2.5 stays.  Ruled out as the
    cause: the gain formula (these gains are near 1, where both forms agree to 4e-3, and a shift gradient, which never
    depended on x-hat, sits at 1.84 x beside them).  What tests/bn_cases.py shows for this trunk size instead: the figures of a
    draw are decided by a handful of ReLU gates that the low-precision forward flips -- the engine flips fewer than the bf16
    oracle but other ones -- and the BatchNorm scale rounded into the bf16 dgrad operand adds up to 1e-2."""
    from magma_amd.testing import build_reduced_magma
    from magma_amd.train_engine import MagmaEngine
    from oracle.model import magma_forward
    L = 4
    cfg = F.full_width_config(n_positions=2048, n_layer=L, enc_width=16, enc_layers=(1, 1, 2, 1))
    params = F.full_depth_params(cfg)
    model = build_reduced_magma(dev, n_layer=L, n_head=16, d_ff=16384, vocab=50258, n_positions=2048)
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing, unexpected)
    model.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(model)
    eng.train()
    B, S, P = 1, 2048, 4
    g = torch.Generator().manual_seed(11)
    images = torch.randn(B, 3, 64, 64, generator=g).to(torch.bfloat16).float()
    caps = torch.full((B, S), cfg.eos_token, dtype=torch.int64)
    caps[0, :67] = torch.randint(0, 50256, (67,), generator=g)
    mask = (torch.rand(B, P, cfg.d_model, generator=g) < 0.9).float() / 0.9
    names = [k for k in params if (".adapter." in k or k.startswith("image_prefix.")) and "running_" not in k]

    def oracle(dtype):
        p = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v) for k, v in params.items()}
        for k in names:
            p[k].requires_grad_(True)
        out = magma_forward(p, cfg, images.to(dtype), F.oracle_window(caps, P, cfg.eos_token), dropout_mask=mask.to(dtype))
        out["loss"].backward()
        return float(out["loss"].detach()), {k: p[k].grad.float() for k in names}

    loss_ref, g_ref = oracle(torch.float32)
    loss_bf, g_bf = oracle(torch.bfloat16)
    out = eng(images.to(dev), caps.to(dev), dropout_mask=mask.to(dev))
    assert abs(float(out.loss) - loss_ref) <= 2 * abs(loss_bf - loss_ref) + 3e-3 * abs(loss_ref), (float(out.loss), loss_ref, loss_bf)
    eng.backward(out.loss)
    name_of = {id(p): n for n, p in model.named_parameters()}
    seen, bad, worst = set(), [], []
    dots = n1 = n2 = bdots = bn1 = 0.0
    per_block = {}
    for grp in eng.groups:
        for p in grp.params:
            n = name_of[id(p)]
            n = "lm." + n if n.startswith("transformer.") else n
            if n in seen or n not in g_ref:
                continue
            seen.add(n)
            got, ref = eng.grad_of(p).float().cpu().reshape(-1), g_ref[n].reshape(-1)
            e_hip, e_bf = rel(got, ref), rel(g_bf[n], ref)
            worst.append((e_hip - 2 * e_bf, n, e_hip, e_bf))
            if ".h." in n:
                li = int(n.split(".h.")[1].split(".")[0])
                per_block[li] = max(per_block.get(li, 0.0), e_hip)
            if e_hip > (2.5 if n.startswith("image_prefix.enc.") else 2.0) * e_bf + 1e-2:
                bad.append((n, e_hip, e_bf))
            dots += float((got * ref).sum()); n1 += float((got * got).sum()); n2 += float((ref * ref).sum())
            gb = g_bf[n].reshape(-1)
            bdots += float((gb * ref).sum()); bn1 += float((gb * gb).sum())
    worst.sort(reverse=True)
    print("loss", float(out.loss), loss_ref, loss_bf, "| worst:", [(n, f"{a:.2e}", f"{b:.2e}") for _, n, a, b in worst[:5]],
          "| worst HIP error per block:", {k: f"{v:.2e}" for k, v in sorted(per_block.items())}, "| tensors", len(seen))
    assert len(seen) == len(g_ref) and set(per_block) == set(range(L)), (len(seen), len(g_ref), sorted(per_block))
    assert not bad, bad[:8]
    cos_hip, cos_bf = dots / (n1 ** 0.5 * n2 ** 0.5), bdots / (bn1 ** 0.5 * n2 ** 0.5)
    print("cosine: hip", cos_hip, "bf16 oracle", cos_bf)
    assert 1 - cos_hip <= 2 * (1 - cos_bf) + 1e-3, (cos_hip, cos_bf)


_FP8_ORACLE_MEMO = {}


@pytest.mark.parametrize("fp8_attn,fp8_mx,fp8_adapters", [(False, False, False), (True, False, False), (True, True, False), (True, True, True)])
def test_fp8_training_step_vs_oracle_on_dequantised_weights(dev, fp8_attn, fp8_mx, fp8_adapters):
    """BASELINE config[4], training side, at full width (d 4096, ff 16384, V 50258, S = 2048, one block, tiny trunk): the engine with
    eng.fp8 = True runs qkv / out_proj / fc_in / fc_out forward AND their dgrads on the fp8 MFMA (e4m3, per-row activation scales,
    per-output-channel weight scales).  Oracle: torch.autograd through the fp32 restatement evaluated on the DEQUANTISED e4m3
    forward weights (what the kernels multiply by) -- not the bf16 HIP step.  What the oracle does not model is the quantisation
    of the ACTIVATIONS / incoming gradients to e4m3 and the separately quantised transposed weights of the dgrads; the stated
    bound is calibrated on the size of the effect that IS modelled: e_w = how far the e4m3 weight quantisation alone moves each
    gradient (oracle on dequantised vs oracle on unquantised weights).
        per tensor   err(HIP fp8, oracle dequantised) <= 2.5 x e_w + 3e-2   (rel-L2; 3 x e_w with the adapter GEMMs in fp8 too)
        all tensors  cosine(HIP fp8, oracle dequantised) >= 0.99;  global err <= 1.5 x global e_w + 1e-2
        loss         within 5e-3 relative of the dequantised oracle's.
    Measured (MI355X, round 4): loss 11.6359 vs 11.6332 (unquantised oracle 11.6310); global error 0.115 where the weight
    quantisation alone moves the gradients by 0.113; cosine 0.9934; worst tensor 0.19 against e_w 0.085 (a BatchNorm gain deep
    in the trunk: the gradient reaches it through all four fp8 dgrads of the block)."""
    from magma_amd.testing import build_reduced_magma
    from magma_amd.train_engine import MagmaEngine
    from oracle.model import attn_prefix, magma_forward, mlp_prefix
    cfg = F.full_width_config(n_positions=2048, enc_width=16, enc_layers=(1, 1, 2, 1))
    params = F.full_width_params(cfg)
    model = build_reduced_magma(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=2048)
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing, unexpected)
    model.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(model)
    eng.fp8 = True
    eng.fp8_attn = fp8_attn       # round 5: QK^T / PV of the attention forward on the fp8 MFMA as well (the oracle does not model it either)
    eng.fp8_adapters = fp8_adapters   # round 6 (BASELINE config[4] "... + adapter GEMMs"): the MLP adapter's down / up GEMMs and their dgrads on the
                                      # fp8 MFMA, operands from the MX output copies of the producing epilogues (train_engine.__init__); the oracle
                                      # keeps the (trainable) adapter weights and every activation exact -- the same bounds hold
    eng.fp8_mx = fp8_mx           # round 5: gelu(fc_in) and its gradient exist only as OCP MX e4m3, written by the GEMM epilogues; fc_out
                                  # and the fc_in dgrad multiply them by MX-quantised weights (whose dequantisation the oracle gets below)
    eng.train()
    B, S, P = 2, 2048, 4
    g = torch.Generator().manual_seed(9)
    images = torch.randn(B, 3, 64, 64, generator=g).to(torch.bfloat16).float()
    caps = torch.full((B, S), cfg.eos_token, dtype=torch.int64)
    caps[0, :53] = torch.randint(0, 50256, (53,), generator=g)
    caps[1, :29] = torch.randint(0, 50256, (29,), generator=g)
    mask = (torch.rand(B, P, cfg.d_model, generator=g) < 0.9).float() / 0.9
    names = [k for k in params if (".adapter." in k or k.startswith("image_prefix.")) and "running_" not in k]
    out = eng(images.to(dev), caps.to(dev), dropout_mask=mask.to(dev))
    loss_hip = float(out.loss)
    eng.backward(out.loss)
    assert bool(eng._ad8_cache) == fp8_adapters            # the fp8 adapter chain ran iff asked for
    packs = eng._fp8_packs
    assert {(0, "qkv"), (0, "out"), (0, "fc_in"), (0, "fc_out"), (0, "qkv_t"), (0, "out_t"), (0, "fc_in_t"), (0, "fc_out_t")} <= set(packs), sorted(packs)
    d = cfg.d_model
    deq = dict(params)
    ap, mp = attn_prefix(cfg, 0), mlp_prefix(cfg, 0)
    w = packs[(0, "qkv")].dequant().cpu()
    deq[ap + "q_proj.weight"], deq[ap + "k_proj.weight"], deq[ap + "v_proj.weight"] = w[:d], w[d:2 * d], w[2 * d:3 * d]
    deq[ap + "out_proj.weight"] = packs[(0, "out")].dequant().cpu()
    deq[mp + "c_fc.weight"] = packs[(0, "fc_in")].dequant().cpu()
    deq[mp + "c_proj.weight"] = packs[(0, "fc_out")].dequant().cpu()

    def oracle(src):
        # the three parametrisations share inputs and most weight sets (unquantised: all three; per-row e4m3: the two non-MX modes
        # and the MX mode's yardstick): each distinct weight set goes through the CPU autograd once per session
        key = tuple((k, float(src[k].double().sum()), float(src[k].double().abs().sum()))
                    for k in (ap + "q_proj.weight", ap + "out_proj.weight", mp + "c_fc.weight", mp + "c_proj.weight"))
        if key in _FP8_ORACLE_MEMO:
            return _FP8_ORACLE_MEMO[key]
        _FP8_ORACLE_MEMO[key] = r = _oracle(src)
        return r

    def _oracle(src):
        p = {k: (v.detach().float().clone() if v.is_floating_point() else v) for k, v in src.items()}
        for k in names:
            p[k].requires_grad_(True)
        o = magma_forward(p, cfg, images, F.oracle_window(caps, P, cfg.eos_token), dropout_mask=mask)
        o["loss"].backward()
        return float(o["loss"].detach()), {k: p[k].grad.float() for k in names}

    loss_deq, g_deq = oracle(deq)
    loss_unq, g_unq = oracle(params)
    g_cal = g_deq
    if fp8_mx:
        # The yardstick e_w stays the one of the other two modes -- how far per-row / per-channel e4m3 weights move each gradient --:
        # it stands for "an fp8 quantisation effect of this size", and the activation / gradient quantisation it is a proxy for
        # did not shrink because two of the eight weight copies are now MX (whose own e_w is smaller: 0.025 against 0.039 on
        # the trunk's BatchNorm gains).  The ORACLE the HIP step is compared with still runs on the weights the kernels multiply by.
        from magma_amd import ops
        cal = dict(deq)
        for key, name in (((0, "fc_out"), mp + "c_proj.weight"),):
            cal[name] = ops.PackedLinearFP8(params[name].to(dev).to(torch.bfloat16)).dequant().cpu()
        _, g_cal = oracle(cal)
    name_of = {id(p): n for n, p in model.named_parameters()}
    seen, bad, rows = set(), [], []
    dot = nh = nr = dw = nu = 0.0
    # per-tensor factor: 2.5 x e_w; with the adapter GEMMs in fp8 as well 3 x e_w -- two more quantised products (the adapter's
    # dgrads, operands MX-quantised by the producing epilogues) sit on the gradient's way down, none of them modelled by the oracle.
    # Measured (MI355X, round 6): worst tensor 0.250 against e_w 0.085 (2.6 x; the same BatchNorm gain deep in the trunk that is
    # worst without: 0.19), loss 11.6479 vs 11.6340, global error 0.134 (weight quantisation alone 0.113), cosine 0.9911 -- the
    # global bounds below are NOT widened.
    k_tensor = 3.0 if fp8_adapters else 2.5
    for grp in eng.groups:
        for p in grp.params:
            n = name_of[id(p)]
            n = "lm." + n if n.startswith("transformer.") else n
            if n in seen or n not in g_deq:
                continue
            seen.add(n)
            got, ref, unq = eng.grad_of(p).float().cpu().reshape(-1), g_deq[n].reshape(-1), g_unq[n].reshape(-1)
            e_hip, e_w = rel(got, ref), rel(g_cal[n].reshape(-1), unq)
            rows.append((e_hip - 2.5 * e_w, n, e_hip, e_w))
            if e_hip > k_tensor * e_w + 3e-2:
                bad.append((n, e_hip, e_w))
            dot += float((got * ref).sum()); nh += float((got * got).sum()); nr += float((ref * ref).sum())
            dw += float(((g_cal[n].reshape(-1) - unq) ** 2).sum()); nu += float(((got - ref) ** 2).sum())
    rows.sort(reverse=True)
    cos = dot / (nh ** 0.5 * nr ** 0.5)
    e_glob, ew_glob = (nu / nr) ** 0.5, (dw / nr) ** 0.5
    print(f"fp8 training step: loss HIP {loss_hip:.5f} oracle(dequantised) {loss_deq:.5f} oracle(unquantised) {loss_unq:.5f} | "
          f"gradients: global err {e_glob:.3e} (weight quantisation alone {ew_glob:.3e}), cosine {cos:.5f}, tensors {len(seen)} | worst:",
          [(n, f"{a:.2e}", f"{b:.2e}") for _, n, a, b in rows[:5]])
    assert len(seen) == len(g_deq), (len(seen), len(g_deq))
    assert abs(loss_hip - loss_deq) <= 5e-3 * abs(loss_deq), (loss_hip, loss_deq, loss_unq)
    # fp8_attn: e4m3 q / k / v^T / P in the attention forward on top (operands the oracle keeps exact) -- the same bounds hold.
    # Measured (MI355X, round 5): loss 11.63929 (11.63592 with the bf16 attention), global error 0.1164 (0.1151), cosine 0.99323 (0.99338).
    assert not bad, bad[:8]
    assert cos >= 0.99 and e_glob <= 1.5 * ew_glob + 1e-2, (cos, e_glob, ew_glob)
