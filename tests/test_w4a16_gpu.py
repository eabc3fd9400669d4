"""W4A16 decode (MAGMA_DECODE_W4): OCP MXFP4 weights -- e2m1 codes, one E8M0 scale per 32 K-elements -- widened to bf16 in the
registers of the weight-streaming GEMVs with the block scale applied.  The widening is exact, so the GEMV is compared BIT FOR BIT
with the bf16 GEMV on the dequantised weights; the engine against the fp32 oracle on the dequantised weights; the public
generate() against the same engine's eager step."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fullwidth_common as F  # noqa: E402
import kernel_compare as kcmp  # noqa: E402

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
TINY_TRUNK = dict(enc_width=16, enc_layers=(1, 1, 2, 1))
WEIGHT_ERR_BAND = (0.10, 0.13)      # relative L2 error of the MX rule on Gaussian weights: 0.118 (tests/test_mxfp4_cpu.py)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def hint(waves, kc, nt):
    return nt | waves << 4 | kc << 8


def rnd(*shape, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


# ------------------------------------------------------------------------------------------------------------ the kernel
def test_every_code_point(dev):
    """K = 512, N = 16: row n holds code n in every position of block 0 and code (n + k) % 16 at position k of the other blocks
    (neighbouring nibbles differ); scale bytes vary per row and block and include both clamp ends (2 and 251).  x is one-hot
    per row, so the fp32 output IS one weight per element: equal to the host table exactly.  Pins the nibble order, the byte
    select of the conversion, and the scale conversion."""
    from magma_amd import ops
    N, K = 16, 512
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    code = torch.where(k < 32, n.expand(N, K), (n + k) % 16).to(torch.uint8)
    codes = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    b = torch.arange(K // 32)[None, :]
    scales = (100 + 3 * n + 5 * b).to(torch.uint8)            # 100 .. 220
    scales[:, 0] = (119 + n[:, 0]).to(torch.uint8)            # block 0: 2^-8 .. 2^7
    scales[:, 2], scales[:, 3], scales[:, 9], scales[:, 14] = 2, 251, 251, 2
    table = ops.dequantize_mx_fp4(codes, scales)              # host table [N, K]
    assert table[3, 0] == 1.5 * 2.0 ** (122 - 127) and table[15, 5] == -6.0 * 2.0 ** (134 - 127)
    lin = ops.PackedLinearW4.__new__(ops.PackedLinearW4)
    lin.N, lin.K, lin.Kp, lin.bias = N, K, K, None
    lin.ft, lin.scales = (t.to(dev) for t in ops.tile_mx_fp4(codes, scales))
    hot = [0, 1, 2, 7, 8, 9, 31, 33, 34, 70, 100, 130, 200, 300, 400, 511]      # every wave's k range, every clamp block
    x = torch.zeros(16, K, dtype=BF16, device=dev)
    x[torch.arange(16), torch.tensor(hot)] = 1.0
    want = table[:, hot].t().contiguous()                     # out[m][n] = W[n][hot[m]]
    for v in (0, hint(4, 4, 1), hint(4, 4, 2)):
        out = ops.gemm_skinny(x, lin, out_dtype=torch.float32, variant=v)
        assert torch.equal(out.cpu(), want), (v, (out.cpu() != want).nonzero()[:8])


SHAPES = [(64, 512), (1000, 4096), (4096, 1024), (256, 16384)]


@pytest.fixture(scope="module")
def packs(dev):
    """One quantised / dequantised operand pair per shape, shared by the M cases."""
    from magma_amd import ops
    made = {}

    def get(N, K):
        if (N, K) not in made:
            w = rnd(N, K, dev=dev, scale=0.05, seed=N + K).to(BF16)
            bias = rnd(N, dev=dev, seed=N + K + 1)
            lin4 = ops.PackedLinearW4(w, bias=bias)
            deq = lin4.dequant()
            assert torch.equal(deq.to(BF16).float(), deq)
            made[(N, K)] = (w, bias, lin4, deq, ops.PackedLinear(deq.to(BF16), bias=bias))
        return made[(N, K)]
    return get


@pytest.mark.parametrize("M", [1, 8, 16])
@pytest.mark.parametrize("N,K", SHAPES)
def test_bit_identical_to_bf16_gemv_on_dequantised_weights(dev, packs, N, K, M):
    """Every W4 variant runs 4 waves, each over a quarter of K in k order; so does the bf16 variant (4 waves, 1 k-step per burst,
    1 n-tile), which divides every K % 128 == 0.  Same bf16 operands into the same MFMA in the same order, the same cross-wave
    sum: torch.equal, for all four shapes (no shape needs the per-element fall-back)."""
    from magma_amd import ops
    w, bias, lin4, deq, lin16 = packs(N, K)
    x = rnd(M, K, dev=dev, seed=M + K).to(BF16)
    ref = ops.gemm_skinny(x, lin16, out_dtype=torch.float32, variant=hint(4, 1, 1))
    kcmp.assert_linear(ref, f"bf16 GEMV on the dequantised weights {N}x{K}", x, deq, bias=bias)
    per_wave = K // 128
    variants = [0] + [hint(4, kc, nt) for kc, nt in ((4, 1), (8, 2), (16, 2), (16, 4), (32, 2), (32, 1)) if per_wave % kc == 0]
    for v in variants:
        out = ops.gemm_skinny(x, lin4, out_dtype=torch.float32, variant=v)
        assert torch.equal(out, ref), (hex(v), rel(out, ref))
    # quantisation is visible: a W4 path that ran unquantised weights would sit at ~0 here
    e = rel(out, x.float() @ w.float().t() + bias)
    e_w = rel(x.float() @ deq.t(), x.float() @ w.float().t())
    print(f"W4A16 {N}x{K} M={M}: rel vs unquantised {e:.4f} (product alone {e_w:.4f})")
    assert WEIGHT_ERR_BAND[0] <= e_w <= WEIGHT_ERR_BAND[1], e_w
    assert rel(out - bias, x.float() @ w.float().t()) == pytest.approx(e_w, rel=1e-2)


@pytest.mark.parametrize("N,K", [(16400, 512), (16400, 1536), (16400, 1024), (8200, 2048)])
def test_default_variants_of_wide_operands_bit_identical(dev, N, K):
    """variant 0 on operands wide enough for several n-tiles per workgroup (1025 n-tiles: four, with bursts of 4 k-steps where a
    wave's share of K is an odd number of k-step quads -- K = 512, 1536 -- and of 8 otherwise; 513 n-tiles: two): the launches
    lm_head and the fused ln_1 + qkv + fc_in operand take by default, against the same bf16 reference."""
    from magma_amd import ops
    w = rnd(N, K, dev=dev, scale=0.05, seed=N + K).to(BF16)
    lin4 = ops.PackedLinearW4(w)
    deq = lin4.dequant()
    x = rnd(8, K, dev=dev, seed=K).to(BF16)
    ref = ops.gemm_skinny(x, ops.PackedLinear(deq.to(BF16)), out_dtype=torch.float32, variant=hint(4, 1, 1))
    kcmp.assert_linear(ref, f"bf16 GEMV on the dequantised weights {N}x{K}", x, deq)
    assert torch.equal(ops.gemm_skinny(x, lin4, out_dtype=torch.float32), ref)
    assert torch.equal(ops.gemm_skinny(x, lin4, out_dtype=torch.float32, variant=hint(4, 4, 4)), ref)


def test_refusals(dev):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    x = rnd(4, 1024, dev=dev).to(BF16)
    lin = ops.PackedLinearW4(rnd(64, 1024, dev=dev, scale=0.05))
    with pytest.raises(MagmaHipError):          # pipelined bursts are bf16-only
        ops.gemm_skinny(x, lin, variant=hint(4, 4, 1) | 1 << 16)
    with pytest.raises(MagmaHipError):          # so is the LDS-DMA GEMV
        ops.gemm_skinny(x, lin, variant=1 << 17)
    with pytest.raises(MagmaHipError):          # 8 waves do not split every K % 512 == 0 in k-step quads
        ops.gemm_skinny(x, lin, variant=hint(8, 4, 1))
    d, _ = ops.skinny_desc(x, lin)
    d.w_scale = lin.scales.data_ptr()           # both weight formats named at once
    with pytest.raises(MagmaHipError):
        ops.check(ops.L.load().mg_gemm_skinny_bf16(ops.C.byref(d), ops._stream()), "mg_gemm_skinny_bf16")
    d, _ = ops.skinny_desc(x, lin)
    d.w_mx4_scale = lin.scales.data_ptr() + 4   # misaligned scales
    with pytest.raises(MagmaHipError):
        ops.check(ops.L.load().mg_gemm_skinny_bf16(ops.C.byref(d), ops._stream()), "mg_gemm_skinny_bf16")
    lin8 = ops.PackedLinearW8(rnd(64, 1024, dev=dev, scale=0.05).to(BF16))
    with pytest.raises(MagmaHipError):          # a pair shares one weight type
        ops.gemm_skinny2((x, lin, None, {}), (x, lin8, None, {}))


def test_layernorm_fold_split_and_pairs(dev):
    from magma_amd import ops
    d, N = 2048, 1000
    x = (rnd(8, d, dev=dev, seed=5) * 2 + 0.3).to(BF16)
    w = rnd(N, d, dev=dev, scale=0.05, seed=6).to(BF16)
    gamma, beta = torch.rand(d, device=dev) + 0.5, rnd(d, dev=dev, seed=7) * 0.1
    w2, b2, _ = ops.fold_layernorm(w, None, gamma, beta)
    lin = ops.PackedLinearW4(w2, bias=b2)
    deq = lin.dequant()
    lin.colsum = deq.sum(1).contiguous()
    out = ops.gemm_skinny(x, lin, ln_fold=(lin.colsum, d, 1e-5), out_dtype=torch.float32)
    xf = x.float()
    mean, var = xf.mean(1, keepdim=True), xf.var(1, unbiased=False, keepdim=True)
    ref = ((xf - mean) * torch.rsqrt(var + 1e-5)) @ deq.t() + b2
    assert rel(out, ref) < 2e-3, rel(out, ref)
    kcmp.assert_elementwise(out, *kcmp.ln_fold_reference(x, deq, b2, lin.colsum, 1e-5, out_dtype=torch.float32), "w4a16 ln-fold GEMV")
    # the same launch with two output segments (qkv | fc_in of the decode block): columns >= 512 with their own bias and ReLU
    oa = torch.empty(8, 512, dtype=torch.float32, device=dev)
    ob = torch.empty(8, N - 512 + 8, dtype=torch.float32, device=dev)[:, : N - 512]
    lin_a = ops.PackedLinearW4.__new__(ops.PackedLinearW4)
    lin_a.__dict__.update(lin.__dict__)
    lin_a.bias = b2[:512].contiguous()
    ops.gemm_skinny(x, lin_a, out=oa, ln_fold=(lin.colsum, d, 1e-5), split=(512, ob, ops.MG_ACT_RELU, b2[512:].contiguous()))
    assert torch.equal(oa, out[:, :512]) and torch.equal(ob, torch.relu(out[:, 512:]))
    # two problems in one launch
    o1 = torch.empty(8, N, dtype=torch.float32, device=dev)
    o2 = torch.empty(8, 512, dtype=torch.float32, device=dev)
    linb = ops.PackedLinearW4(rnd(512, d, dev=dev, scale=0.05, seed=8).to(BF16))
    ops.gemm_skinny2((x, lin, o1, {}), (x, linb, o2, {"act": ops.MG_ACT_RELU}))
    kcmp.assert_linear(o1, "w4a16 pair, first problem", x, deq, bias=b2)
    kcmp.assert_linear(o2, "w4a16 pair, second problem (relu)", x, linb.dequant(), act="relu")
    # 4 waves in k order again: the pair equals the single launches bit for bit
    assert torch.equal(o1, ops.gemm_skinny(x, lin, out_dtype=torch.float32))
    assert torch.equal(o2, ops.gemm_skinny(x, linb, out_dtype=torch.float32, act=ops.MG_ACT_RELU))
    # a pair whose K differ (out_proj || adapter-down shapes): K = 2048 and K = 512 (the 4-k-step bursts)
    xs = rnd(8, 512, dev=dev, seed=9).to(BF16)
    lins = ops.PackedLinearW4(rnd(100, 512, dev=dev, scale=0.05, seed=10).to(BF16))
    o3 = torch.empty(8, 104, dtype=torch.float32, device=dev)[:, :100]
    ops.gemm_skinny2((x, lin, o1, {}), (xs, lins, o3, {}))
    assert torch.equal(o1, ops.gemm_skinny(x, lin, out_dtype=torch.float32))
    assert torch.equal(o3, ops.gemm_skinny(xs, lins, out_dtype=torch.float32))


@pytest.mark.parametrize("K", [512, 1024, 2048])
def test_attention_co_launch(dev, K):
    """decode_attn_gemv at H = 4, context 64 with a W4 GEMV (K picks each of its three burst depths: 4, 8, 16 k-steps): the attention part writes
    what the stand-alone launch writes, the GEMV part what the stand-alone W4 GEMV gives, bit for bit."""
    from magma_amd import ops
    from oracle.model import rotary_tables
    B, H, Smax, rot, N = 3, 4, 128, 64, 1000
    d = H * 256
    kc0 = rnd(B, H, Smax, 256, dev=dev, seed=11, scale=0.5).to(BF16)
    vc0 = rnd(B, H, Smax, 256, dev=dev, seed=12).to(BF16)
    qkv = rnd(B, 3 * d, dev=dev, seed=13, scale=0.5).to(BF16)
    sin_t, cos_t = (t.to(dev).contiguous() for t in rotary_tables(rot, Smax))
    d_pos = torch.tensor([64], dtype=torch.int32, device=dev)
    kc, vc, out = kc0.clone(), vc0.clone(), torch.empty(B, d, dtype=BF16, device=dev)
    ops.attn_decode_fused(qkv, kc, vc, out, B, H, d_pos, rot, sin_t, cos_t)
    xg = rnd(B, K, dev=dev, seed=14).to(BF16)
    lin = ops.PackedLinearW4(rnd(N, K, dev=dev, seed=15, scale=0.05).to(BF16), bias=rnd(N, dev=dev, seed=16))
    y = torch.empty(B, N, dtype=torch.float32, device=dev)
    kc2, vc2, out2 = kc0.clone(), vc0.clone(), torch.empty(B, d, dtype=BF16, device=dev)
    ops.decode_attn_gemv(qkv, kc2, vc2, out2, B, H, d_pos, rot, sin_t, cos_t, (xg, lin, y, {"out_dtype": torch.float32}))
    assert torch.equal(kc2, kc) and torch.equal(vc2, vc) and torch.equal(out2, out)
    assert torch.equal(y, ops.gemm_skinny(xg, lin, out_dtype=torch.float32))
    kcmp.assert_linear(y, f"co-launched W4 GEMV, K = {K}", xg, lin.dequant(), bias=lin.bias)


# ------------------------------------------------------------------------------------------------------------ the engine
def no_ln_bias(params):
    """LayerNorm biases zeroed: with beta = 0 the LayerNorm fold of the decode operands (W' = W * gamma, then quantised) is EXACTLY
    'the oracle on the weights dequant(W') / gamma'."""
    p = dict(params)
    for k in p:
        if k.endswith("ln_1.bias") or k.endswith("ln_f.bias"):
            p[k] = torch.zeros_like(p[k])
    return p


def build(dev, cfg, params, **kw):
    from magma_amd.testing import build_reduced_magma
    model = build_reduced_magma(dev, n_layer=cfg.n_layer, n_head=16, d_ff=16384, vocab=50258, n_positions=cfg.n_positions,
                                enc_width=cfg.enc_width, enc_layers=cfg.enc_layers, resolution=64, **kw)
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing[:4], unexpected[:4])
    model.eval()
    return model


def margin_safe(ref_logits):
    top2 = torch.topk(ref_logits, 2, dim=-1).values
    return (top2[:, 0] - top2[:, 1]) > F.TEST_MARGIN * ref_logits.std(dim=-1)


def test_w4a16_decode_vs_oracle_on_dequantised_weights(dev):
    """W4A16 token step at full width, one block, against the fp32 oracle evaluated on the engine's own dequantised operands, from
    the SAME bf16 prefill cache.  What is left between the two is bf16 activation rounding only: 2 x eager-bf16 criterion (floor
    3e-3); quantisation itself moves the logits by more than 5 x that residual, so unquantised weights would be noticed."""
    from oracle.model import attn_prefix, lm_forward, mlp_adapter_prefix, mlp_prefix
    cfg = F.full_width_config(**TINY_TRUNK)
    p = no_ln_bias(F.full_width_params(cfg))
    model = build(dev, cfg, p)
    eng = model.lm.engine
    lm = F.lm_only(p)
    emb = F.greedy_inputs(cfg, seed=97, B=8, S0=16)
    bf16_params = lambda s: {k: (v.to(BF16) if v.is_floating_point() else v) for k, v in s.items()}  # noqa: E731
    try:
        eng.decode_w4 = True
        with torch.no_grad():
            r0 = lm_forward(lm, cfg, inputs_embeds=emb)
            out = model.lm(inputs_embeds=emb.to(BF16).cuda(), use_cache=True, cache_hint=8)     # prefill: bf16 weights
            tok = r0["logits"][:, -1].argmax(-1, keepdim=True)
            o = model.lm(input_ids=tok.cuda(), use_cache=True, past_key_values=out.past_key_values)
            ly = eng.layers[0]
            assert getattr(ly, "w4", None) is not None and ly.w8 is None, "the W4A16 operands were not built: the MXFP4 path did not run"
            assert out.past_key_values.decode_state.w4 and out.past_key_values.decode_state.kinds == ["grouped"]
            d, d3 = cfg.d_model, 3 * cfg.d_model
            q = dict(lm)
            gam = lm["lm.transformer.h.0.ln_1.weight"]
            w_in = ly.w4.dec_in.dequant().cpu() / gam[None, :]
            ap, mp, adp = attn_prefix(cfg, 0), mlp_prefix(cfg, 0), mlp_adapter_prefix(cfg, 0)
            q[ap + "q_proj.weight"], q[ap + "k_proj.weight"], q[ap + "v_proj.weight"] = w_in[:d], w_in[d:2 * d], w_in[2 * d:d3]
            q[mp + "c_fc.weight"] = w_in[d3:]
            q[ap + "out_proj.weight"] = ly.w4.out.dequant().cpu()
            q[mp + "c_proj.weight"] = ly.w4.fc_out.dequant().cpu()
            q[adp + "0.weight"] = ly.w4.mlp_adapter[0].dequant().cpu()
            q[adp + "2.weight"] = ly.w4.mlp_adapter[1].dequant().cpu()
            q["lm.lm_head.weight"] = eng.head_w4.dequant().cpu()[: cfg.vocab_out] / lm["lm.transformer.ln_f.weight"][None, :]
            # the engine quantised what the CPU restatement quantises
            from magma_amd import ops
            mine = ops.dequantize_mx_fp4(*ops.quantize_mx_fp4(lm[adp + "2.weight"].to(BF16)))
            assert torch.equal(mine, q[adp + "2.weight"])
            r = lm_forward(q, cfg, input_ids=tok, past=r0["past_key_values"])
            rb = lm_forward(bf16_params(q), cfg, input_ids=tok, past=[(k.to(BF16), v.to(BF16)) for k, v in r0["past_key_values"]])
            ref = r["logits"][:, -1]
            e_hip, e_bf = rel(o.logits[:, -1], ref), rel(rb["logits"][:, -1], ref)
            print(f"W4A16 step logits vs dequantised oracle: HIP err {e_hip:.3e}, eager-bf16 err {e_bf:.3e}")
            assert e_hip <= 2.0 * e_bf + 3e-3, (e_hip, e_bf)
            unq = lm_forward(lm, cfg, input_ids=tok, past=r0["past_key_values"])["logits"][:, -1]
            print("MXFP4 weight quantisation itself moves the logits by", rel(ref, unq))
            assert rel(ref, unq) > 5 * e_hip, "the comparison would not notice unquantised weights"
            safe = margin_safe(ref)
            assert bool((o.next_token.cpu()[safe] == ref.argmax(-1)[safe]).all())
    finally:
        eng.decode_w4 = False
        eng._cache_pool.clear()


# config name -> (oracle config of the adapters, build_reduced_magma arguments)
STEP_CASES = {"MAGMA_v1": ({}, {}),
              "MAGMA_v2": (dict(mlp_adapter_hidden=512, attn_adapter_hidden=512), dict(mlp_factor=8, attn_factor=8))}
# rel-L2 between the fp32 oracle's step logits on the dequantised and on the original weights (2 blocks, full width, B = 8,
# 16-token prefill, seed 97): printed by `python tools/w4_step_quant_shift.py`, a CPU-only fp32 computation (about a minute per
# config, which is why the test carries its result and does not repeat it)
STEP_QUANT_SHIFT = {"MAGMA_v1": 0.2474, "MAGMA_v2": 0.2393}


@pytest.mark.parametrize("config", list(STEP_CASES))
def test_w4a16_step_tracks_bf16(dev, config):
    """Full-width 2-block MAGMA_v1 / MAGMA_v2: the greedy W4A16 step stays as close to the bf16 step as weight quantisation allows.
    The bound is NOT taken from the kernels: STEP_QUANT_SHIFT is rel-L2(oracle(dequantised weights), oracle(original weights)) of
    the same step's logits, computed on the CPU in fp32 (tools/w4_step_quant_shift.py regenerates it: same weights, inputs and prefill
    length as here);
    the engine's two modes may differ by 1.5 x that (the margin covers the bf16 activation rounding of both runs).
    Measured on the CPU: 0.2474 (MAGMA_v1), 0.2393 (MAGMA_v2) -- large because the weights are random; on an MI355X the engine's
    two modes then differed by 0.2475 and 0.2393."""
    from oracle.model import lm_forward
    ckw, bkw = STEP_CASES[config]
    cfg = F.full_width_config(n_layer=2, **ckw, **TINY_TRUNK)
    p = no_ln_bias(F.full_width_params(cfg))
    model = build(dev, cfg, p, **bkw)
    eng = model.lm.engine
    emb = F.greedy_inputs(cfg, seed=97, B=8, S0=16)
    logits, toks = {}, {}
    try:
        with torch.no_grad():
            for mode in (False, True):
                eng.decode_w4 = mode
                eng._cache_pool.clear()
                pre = model.lm(inputs_embeds=emb.to(BF16).cuda(), use_cache=True, cache_hint=8)
                tok = pre.logits[:, -1].argmax(-1, keepdim=True)
                step = model.lm(input_ids=tok, use_cache=True, past_key_values=pre.past_key_values)
                logits[mode], toks[mode] = step.logits[:, -1].float().clone(), step.next_token.clone()
                assert pre.past_key_values.decode_state.w4 == mode
            kinds = pre.past_key_values.decode_state.kinds
    finally:
        eng.decode_w4 = False
        eng._cache_pool.clear()
    assert kinds == [{"MAGMA_v1": "grouped", "MAGMA_v2": "v2"}[config]] * 2, kinds
    e = rel(logits[True], logits[False])
    print(f"{config}: W4A16 vs bf16 step logits rel-L2 {e:.4f}; oracle-measured quantisation shift {STEP_QUANT_SHIFT[config]}")
    assert e <= 1.5 * STEP_QUANT_SHIFT[config], (e, STEP_QUANT_SHIFT[config])
    assert e > 0.2 * STEP_QUANT_SHIFT[config], "W4A16 changed next to nothing: the MXFP4 operands were not used"
    assert torch.equal(toks[True], logits[True].argmax(-1)) and torch.equal(toks[False], logits[False].argmax(-1))


# ------------------------------------------------------------------------------------------------------------ generate()
N_STEPS = 6


def _model(dev, monkeypatch, switch="MAGMA_DECODE_W4", mlp_factor=2, **kw):
    """Two blocks, d 1024 (4 heads), ff 2048, adapter bottleneck 512: every decode operand has K % 512 == 0."""
    from magma_amd.testing import build_reduced_magma
    monkeypatch.setenv(switch, "1")
    torch.manual_seed(0)
    model = build_reduced_magma(dev, n_layer=2, n_head=4, d_ff=2048, mlp_factor=mlp_factor, **kw)
    model.eval()
    with torch.no_grad():       # eos within reach
        model.lm.lm_head.bias[model.eos_token] += 4.0
        model.lm.invalidate_packed()
    assert model.lm.engine.decode_w4 == (switch == "MAGMA_DECODE_W4") and model.lm.engine.decode_w8 != model.lm.engine.decode_w4
    return model


def _emb(model, B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, model.lm.config.hidden_size, generator=g).to(BF16).to(model.device)


def _rows(out, S, n, lengths):
    if lengths is None:
        return out[:, S: S + n].cpu()
    return torch.stack([out[i, int(m): int(m) + n].cpu() for i, m in enumerate(lengths)])


def _eager_greedy(model, emb, n, lengths=None, rules=None):
    """prefill + eager (un-captured) W4A16 steps fed the host's argmax of the (host-processed) logits."""
    from magma_amd.sampling import process_logits
    eng = model.lm.engine
    kw = {} if lengths is None else {"lengths": torch.as_tensor(lengths)}
    o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=n, **kw)
    c = o.past_key_values
    lg = o.logits[:, -1].float().cpu()
    hist = torch.zeros(emb.shape[0], n, dtype=torch.int64)
    for t in range(n):
        x = lg if rules is None else process_logits(lg, hist, t, eos_token=model.eos_token, **rules)
        hist[:, t] = x.argmax(-1)
        if t + 1 < n:
            lg = eng.decode(hist[:, t:t + 1].to(model.device), c, use_graph=False)[0].float().cpu()
    st = c.decode_state
    assert st.w4 and not st.w8 and st.refusal is None and st.kinds == ["grouped"] * 2
    return hist


def test_generate_ragged_batch(dev, monkeypatch):
    model = _model(dev, monkeypatch)
    S, lengths = 7, [7, 4, 5]
    emb = _emb(model, 3, S, seed=41)
    out = model.generate(emb, max_steps=N_STEPS, temperature=0.0, decode=False, stop_on_eos=False, lengths=lengths)
    assert torch.equal(_rows(out, S, N_STEPS, lengths), _eager_greedy(model, emb, N_STEPS, lengths))


def test_generate_logits_processors(dev, monkeypatch):
    model = _model(dev, monkeypatch)
    S = 7
    emb = _emb(model, 3, S, seed=42)
    kw = dict(max_steps=N_STEPS, temperature=0.0, decode=False, stop_on_eos=False)
    plain = _rows(model.generate(emb, **kw), S, N_STEPS, None)
    assert torch.equal(plain, _eager_greedy(model, emb, N_STEPS))
    emitted = [t for t in dict.fromkeys(plain.flatten().tolist()) if t != model.eos_token]
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=1, min_new_tokens=3, suppress_tokens=tuple(emitted[:2]) or (model.eos_token,))
    got = _rows(model.generate(emb, **kw, **rules), S, N_STEPS, None)
    assert torch.equal(got, _eager_greedy(model, emb, N_STEPS, rules=rules)), (rules, got)
    assert not torch.equal(got, plain)


def test_generate_beam_search(dev, monkeypatch):
    from magma_amd.sampling import beam_search
    model = _model(dev, monkeypatch)
    eng = model.lm.engine
    B, S, k, n = 2, 6, 3, 8
    emb = _emb(model, B, S, seed=43)
    box = {}

    def step(rows, tokens):
        if rows is None:
            o = eng.forward(inputs_embeds=emb.repeat_interleave(k, dim=0), use_cache=True, cache_hint=n)
            box["c"] = o.past_key_values
            return o.logits[:, -1].float().cpu()
        c, r = box["c"], rows.to(dev)
        c.k.copy_(c.k.index_select(1, r))
        c.v.copy_(c.v.index_select(1, r))
        return eng.decode(tokens.view(-1, 1).to(dev), c, use_graph=False)[0].float().cpu()

    ref_seq, ref_sc, _ = beam_search(step, B, k, n, model.eos_token, 1.0, False, k)
    assert box["c"].decode_state.w4
    out, sc = model.generate(emb, max_steps=n, num_beams=k, num_return_sequences=k, decode=False, return_scores=True)
    assert torch.equal(out[:, S:].cpu(), ref_seq), (out[:, S:], ref_seq)
    assert torch.allclose(sc, ref_sc, rtol=1e-5, atol=1e-5), (sc, ref_sc)


def test_wide_batch_is_refused_and_both_modes_raise(dev, monkeypatch):
    """B = 17: the plan refuses W4A16 with its reason before anything is enqueued, as W8A16 does (decode() raises; a caller
    that wants the tile-GEMM step switches the mode off); decode_w4 and decode_w8 together are an error."""
    model = _model(dev, monkeypatch)
    eng = model.lm.engine
    emb = _emb(model, 17, 5, seed=44)
    with torch.no_grad():
        o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=4)
        tok = o.logits[:, -1].argmax(-1, keepdim=True)
        with pytest.warns(RuntimeWarning), pytest.raises(NotImplementedError, match="W4A16 decode covers batches of at most 16 sequences"):
            eng.decode(tok, o.past_key_values)
        eng.decode_w4 = False                     # the fall-back of W8A16: the bf16 tile-GEMM step on a fresh cache
        eng._cache_pool.clear()
        o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=4)
        lg, _ = eng.decode(tok, o.past_key_values)
        assert torch.isfinite(lg).all()
        eng.decode_w4 = eng.decode_w8 = True
        eng._cache_pool.clear()
        o = eng.forward(inputs_embeds=emb[:2], use_cache=True, cache_hint=4)
        with pytest.raises(ValueError, match="decode_w8 .* and decode_w4"):
            eng.decode(tok[:2], o.past_key_values)
    eng.decode_w4 = eng.decode_w8 = False
    monkeypatch.setenv("MAGMA_DECODE_W8", "1")
    with pytest.raises(ValueError, match="decode_w8 .* and decode_w4"):
        model.lm.invalidate_packed()
        model.lm.engine


def test_adapter_k_that_does_not_fit_is_refused(dev, monkeypatch):
    """An adapter bottleneck of 256 (K of the up-projection) has no MXFP4 operand: the step is refused with the reason."""
    from magma_amd.testing import build_reduced_magma
    monkeypatch.setenv("MAGMA_DECODE_W4", "1")
    torch.manual_seed(0)
    model = build_reduced_magma(dev, n_layer=1, n_head=4, d_ff=2048, mlp_factor=4)
    model.eval()
    eng = model.lm.engine
    with torch.no_grad():
        o = eng.forward(inputs_embeds=_emb(model, 2, 5, seed=45), use_cache=True, cache_hint=4)
        with pytest.raises(NotImplementedError, match="W4A16 decode needs adapter projections with K % 512 == 0"):
            eng.decode(o.logits[:, -1].argmax(-1, keepdim=True), o.past_key_values)
    assert o.past_key_values.decode_state.refusal is not None


@pytest.mark.parametrize("fmt", ["w4", "w8"])
def test_repack_adapters_requantises_the_adapter_operands(dev, monkeypatch, fmt):
    """After the adapter weights change, repack_adapters leaves the quantised copies of the adapter projections current (MXFP4,
    and the e4m3 ones built by the same helper; bottleneck 1024 for W8A16's K % 1024): the step computes what a freshly built
    engine computes."""
    model = _model(dev, monkeypatch) if fmt == "w4" else _model(dev, monkeypatch, switch="MAGMA_DECODE_W8", mlp_factor=1)
    emb = _emb(model, 2, 5, seed=46)

    def step():
        eng = model.lm.engine
        eng._cache_pool.clear()
        o = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=4)
        tok = torch.full((2, 1), 7, dtype=torch.int64, device=dev)
        lg = eng.decode(tok, o.past_key_values, use_graph=False)[0].float().clone()
        assert getattr(o.past_key_values.decode_state, fmt) and getattr(eng.layers[0], fmt) is not None
        return lg

    with torch.no_grad():
        before = step()
        eng = model.lm.engine
        for name, p in model.lm.named_parameters():
            if ".adapter." in name and name.endswith("weight"):
                p.mul_(1.5)
        eng.repack_adapters(model.lm)
        after = step()
        assert model.lm.engine is eng
        model.lm.invalidate_packed()
        fresh = step()
    assert torch.equal(after, fresh) and not torch.equal(before, after)


def test_frozen_k_that_does_not_fit_is_refused(dev, monkeypatch):
    """d = 768 (3 heads): the frozen projections themselves have no MXFP4 operand.  Nothing is packed, the plan carries the reason
    and decode() raises it before the step's first launch; the bf16 step of the same engine still runs."""
    from magma_amd.testing import build_reduced_magma
    monkeypatch.setenv("MAGMA_DECODE_W4", "1")
    torch.manual_seed(0)
    model = build_reduced_magma(dev, n_layer=1, n_head=3, d_ff=2048, mlp_factor=3)
    model.eval()
    eng = model.lm.engine
    with torch.no_grad():
        o = eng.forward(inputs_embeds=_emb(model, 2, 5, seed=47), use_cache=True, cache_hint=4)
        tok = o.logits[:, -1].argmax(-1, keepdim=True)
        with pytest.raises(NotImplementedError, match="W4A16 decode needs every projection's K to be a multiple of 512 .*768"):
            eng.decode(tok, o.past_key_values)
        assert "768" in o.past_key_values.decode_state.refusal and eng.head_w4 is None and eng.layers[0].w4 is None
        eng.decode_w4 = False
        eng._cache_pool.clear()
        o = eng.forward(inputs_embeds=_emb(model, 2, 5, seed=47), use_cache=True, cache_hint=4)
        assert torch.isfinite(eng.decode(tok, o.past_key_values)[0]).all()
