"""Backward / optimizer kernels against torch autograd (fp32) on the same inputs."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_compare as kcmp

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def rnd(*shape, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def rot_tables(rows, rot, dev):
    """fp32 GPT-J tables sin, cos [rows, rot / 2] (rot = 0: empty tables, which the entry points accept)."""
    inv = 1.0 / (10000 ** (torch.arange(0, rot, 2, dtype=torch.float32, device=dev) / max(rot, 1)))
    ang = torch.arange(rows, dtype=torch.float32, device=dev)[:, None] * inv[None, :]
    return ang.sin().contiguous(), ang.cos().contiguous()


def test_transposes(dev):
    from magma_amd import ops
    x = rnd(200, 136, dev=dev, seed=1).to(BF16)
    assert torch.equal(ops.transpose(x), x.t().contiguous())
    y = rnd(13, 16, dev=dev, seed=1).to(BF16)                       # R not a multiple of 8 -> zero padded columns
    yt = ops.transpose(y)
    assert yt.shape == (16, 16) and torch.equal(yt[:, :13], y.t()) and bool((yt[:, 13:] == 0).all())
    B, H, S = 2, 3, 57
    src = rnd(B * S, H * 256, dev=dev, seed=2).to(BF16)          # [M, d] activation -> per-head transposed
    out = ops.head_transpose(src, B, H, S, sb=S * H * 256, ss=H * 256, sh=256)
    def untile(t):     # [B,H,T,256,32] column-tiled -> [B,H,256,T*32]
        return t.permute(0, 1, 3, 2, 4).reshape(t.shape[0], t.shape[1], 256, -1)
    ref = src.view(B, S, H, 256).permute(0, 2, 3, 1)
    assert out.shape == (B, H, 2, 256, 32)
    assert torch.equal(untile(out)[..., :S], ref) and bool((untile(out)[..., S:] == 0).all())
    q = rnd(B, H, S, 256, dev=dev, seed=3).to(BF16)               # [B,H,S,256] -> [B,H,256,S]
    out = ops.head_transpose(q, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    assert torch.equal(untile(out)[..., :S], q.transpose(2, 3))


def test_colsum(dev):
    from magma_amd import ops
    x = rnd(1000, 520, dev=dev, seed=4).to(BF16)
    y = rnd(1000, 520, dev=dev, seed=5).to(BF16)
    out = torch.zeros(520, device=dev)
    ops.colsum(x, out)
    assert rel(out, x.float().sum(0)) < 1e-5
    s1, m1 = x.double().sum(0), x.double().abs().sum(0)
    kcmp.assert_elementwise(out, s1, kcmp.rounded(s1, kcmp.gamma(1000 + 8) * m1, torch.float32), "colsum")
    first = out.clone()
    ops.colsum(x, out, y)                                         # accumulates
    assert rel(out, x.float().sum(0) + (x.float() * y.float()).sum(0)) < 1e-5
    s2, m2 = first.double() + (x.double() * y.double()).sum(0), first.double().abs() + (x.double() * y.double()).abs().sum(0)
    kcmp.assert_elementwise(out, s2, kcmp.rounded(s2, kcmp.gamma(1000 + 9) * m2, torch.float32), "colsum of x * y, accumulated")


@pytest.mark.parametrize("M,N", [(8, 64), (300, 40), (2085, 520)])
def test_colsum_deterministic(dev, M, N):
    """The two-stage form the batch-statistics BatchNorm uses: 1, 2 and 9 partials of 256 rows (the last one short), one and two
    column stripes of 512.  Same fp64 reference and the same bound as test_colsum (M terms in some order, the accumulation, the
    partials' extra additions); it accumulates into what ``out`` holds, and -- its point -- repeated calls give the same bits
    whatever order the workgroups retire in (the atomic form does not from three partials on)."""
    from magma_amd import ops
    x = rnd(M, N, dev=dev, seed=40).to(BF16)
    y = rnd(M, N, dev=dev, seed=41).to(BF16)
    start = rnd(N, dev=dev, seed=42)
    s1, m1 = x.double().sum(0), x.double().abs().sum(0)
    out = torch.zeros(N, device=dev)
    ops.colsum(x, out, deterministic=True)
    kcmp.assert_elementwise(out, s1, kcmp.rounded(s1, kcmp.gamma(M + 9) * m1, torch.float32), f"deterministic colsum {M}x{N}")
    xy = x.double() * y.double()
    s2, m2 = start.double() + xy.sum(0), start.double().abs() + xy.abs().sum(0)
    runs = []
    for _ in range(8):
        out = start.clone()
        ops.colsum(x, out, y, deterministic=True)
        runs.append(out)
    kcmp.assert_elementwise(runs[0], s2, kcmp.rounded(s2, kcmp.gamma(M + 9) * m2, torch.float32), f"deterministic colsum of x * y {M}x{N}, accumulated")
    assert all(torch.equal(r, runs[0]) for r in runs[1:])


@pytest.mark.parametrize("rows,d", [(9, 4096), (33, 512)])
def test_layernorm_bwd(dev, rows, d):
    from magma_amd import ops
    x = (rnd(rows, d, dev=dev, seed=6) * 2 + 0.5).to(BF16)
    dy = rnd(rows, d, dev=dev, seed=7).to(BF16)
    res = rnd(rows, d, dev=dev, seed=8).to(BF16)
    g = rnd(d, dev=dev, seed=9) * 0.1 + 1
    xf = x.float().requires_grad_(True)
    yref = F.layer_norm(xf, (d,), g, torch.zeros(d, device=dev), 1e-5)
    yref.backward(dy.float())
    dx, xh = ops.layernorm_bwd(dy, x, g, 1e-5, res=res, want_xhat=True)
    assert rel(dx, xf.grad + res.float()) < 4e-3
    assert rel(xh, F.layer_norm(x.float(), (d,))) < 4e-3
    R = kcmp.layernorm_bwd_reference(dy, x, g, 1e-5, res=res)
    kcmp.assert_elementwise(dx, *R["dx"], f"layernorm_bwd dx {rows}x{d}")
    kcmp.assert_elementwise(xh, *R["xhat"], f"layernorm_bwd xhat {rows}x{d}")


def test_ce_fwd_bwd(dev):
    from magma_amd import ops
    R, V = 21, 1053
    lg = (rnd(R, V, dev=dev, seed=10) * 3)
    tg = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(1))
    tg[::4] = -100
    lgr = lg.clone().requires_grad_(True)
    ref = F.cross_entropy(lgr, tg.to(dev), ignore_index=-100)
    ref.backward()
    loss, dl = ops.cross_entropy_fwd_bwd(lg, tg.to(dev), 1056)
    assert abs(float(loss) - float(ref)) < 1e-4
    assert rel(dl[:, :V], lgr.grad) < 4e-3 and bool((dl[:, V:] == 0).all())
    kcmp.assert_elementwise(dl[:, :V], *kcmp.cross_entropy_reference(lg, tg)["dlogits"], "cross-entropy d logits")


def test_epilogue_aux_modes(dev):
    from magma_amd import ops
    M, N, K = 130, 264, 128
    a = rnd(M, K, dev=dev, seed=11).to(BF16)
    w = rnd(N, K, dev=dev, seed=12, scale=0.1).to(BF16)
    aux = rnd(M, N, dev=dev, seed=13).to(BF16)
    r0 = rnd(M, N, dev=dev, seed=14).to(BF16)
    lin = ops.PackedLinear(w, bias=rnd(N, dev=dev, seed=15))
    acc = a.float() @ w.float().t() + lin.bias
    # per element: the accumulator A W^T + bias in fp64 with its fp32 error (a bound without an output rounding), then what
    # each aux mode does to it -- a product with a factor f multiplies the error by |f| and rounds once more
    acc64, acc_err = kcmp.linear_reference(a, w, bias=lin.bias, out_dtype=torch.float64)
    gate = (aux.double() > 0).double()
    U = kcmp.U_F32

    def bound(ref, err):
        return kcmp.rounded(ref, err, BF16)
    out = ops.gemm(a, lin, aux=aux, aux_mode=ops.MG_AUX_RELU_GATE, residuals=(r0,))
    assert rel(out, acc * (aux.float() > 0) + r0.float()) < 4e-3
    ref = acc64 * gate + r0.double()
    kcmp.assert_elementwise(out, ref, bound(ref, acc_err * gate + U * ((acc64 * gate).abs() + r0.double().abs())), "aux relu gate, then residual")
    out = ops.gemm(a, lin, aux=aux, aux_mode=ops.MG_AUX_RELU_GATE, residuals=(r0,), aux_after=True)
    assert rel(out, (acc + r0.float()) * (aux.float() > 0)) < 4e-3
    ref = (acc64 + r0.double()) * gate
    kcmp.assert_elementwise(out, ref, bound(ref, (acc_err + U * (acc64.abs() + r0.double().abs())) * gate), "residual, then aux relu gate")
    xa = aux.float().requires_grad_(True)
    gl = 0.5 * xa * (1 + torch.tanh(math.sqrt(2 / math.pi) * (xa + 0.044715 * xa ** 3)))
    gl.sum().backward()
    out = ops.gemm(a, lin, aux=aux, aux_mode=ops.MG_AUX_GELU_GRAD)
    assert rel(out, acc * xa.grad) < 4e-3
    gg, gg_err = kcmp.gelu_new_grad_terms(aux)
    ref = acc64 * gg
    kcmp.assert_elementwise(out, ref, bound(ref, acc_err * gg.abs() + acc64.abs() * gg_err + U * ref.abs()), "aux gelu gradient")
    out = ops.gemm(a, lin, aux=aux, aux_mode=ops.MG_AUX_MUL)
    assert rel(out, acc * aux.float()) < 4e-3
    ref = acc64 * aux.double()
    kcmp.assert_elementwise(out, ref, bound(ref, acc_err * aux.double().abs() + U * ref.abs()), "aux multiply")
    pre = torch.empty(M, N, dtype=BF16, device=dev)
    out = ops.gemm(a, lin, act=ops.MG_ACT_GELU_NEW, out2=pre)
    assert rel(pre, acc) < 4e-3 and rel(out, F.gelu(acc, approximate="tanh")) < 4e-3
    kcmp.assert_linear(pre, "pre-activation copy (out2)", a, w, bias=lin.bias)
    kcmp.assert_linear(out, "gelu beside the pre-activation copy", a, w, bias=lin.bias, act="gelu")


@pytest.mark.parametrize("B,H,S", [(1, 1, 64), (2, 2, 57), (1, 2, 152), (1, 1, 1), (1, 2, 300), (2, 1, 385), (1, 1, 1024)])
def test_attention_backward(dev, B, H, S):
    from magma_amd import ops
    d = H * 256
    q = rnd(B, H, S, 256, dev=dev, seed=20, scale=0.5).to(BF16)
    k = rnd(B, H, S, 256, dev=dev, seed=21, scale=0.5).to(BF16)
    v = rnd(B, H, S, 256, dev=dev, seed=22).to(BF16)
    dO = rnd(B * S, d, dev=dev, seed=23).to(BF16)
    vt = ops.head_transpose(v, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    out = torch.empty(B * S, d, dtype=BF16, device=dev)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
    ops.attn_prefill(q, k, vt, out, B, H, S, lse=lse)
    qt = ops.head_transpose(q, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    kt = ops.head_transpose(k, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    dOt = ops.head_transpose(dO, B, H, S, sb=S * d, ss=d, sh=256)
    dq, dk, dv = ops.attn_bwd(q, k, v, qt, kt, dO, dOt, out, lse, B, H, S)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    sc = qf @ kf.transpose(-1, -2) / 16.0
    sc = sc.masked_fill(~torch.ones(S, S, dtype=torch.bool, device=dev).tril(), float("-inf"))
    o = (torch.softmax(sc, -1) @ vf).permute(0, 2, 1, 3).reshape(B * S, d)
    o.backward(dO.float())
    for got, ref, name in ((dq, qf.grad, "dq"), (dk, kf.grad, "dk"), (dv, vf.grad, "dv")):
        if float(ref.abs().max()) < 1e-6:      # S = 1: softmax over one key has zero gradient
            assert float(got.float().abs().max()) < 1e-6, name
        else:
            assert rel(got, ref) < 1.5e-2, (name, rel(got, ref))
    kcmp.assert_causal_attention(out, q, k, v, f"prefill attention (forward of the backward test) B={B} H={H} S={S}", lse=lse)
    kcmp.assert_attention_backward(dq, dk, dv, q, k, v, dO, out, lse, f"attn_bwd B={B} H={H} S={S}")


@pytest.mark.parametrize("inputs", ["self c=1", "self c=2", "tile edges"])
@pytest.mark.parametrize("S", [57, 300, 385, 1024, 2048])
def test_attention_backward_boundary_inputs(dev, S, inputs):
    """dQ / dK / dV of attn_bwd and attn_bwd_rows (and the forward of attn_fwd_rows) on inputs where the causal boundary counts:
    each query's own key dominates its row, or the keys at the edges of the 32-key tiles and the last key do
    (kernel_compare.self_dominant_qkv / dominant_edge_keys); partial (57 / 300 / 385) and full (1024 / 2048) last tiles.  dV_j is
    sum_i P_ij dO_i: a diagonal weight that is left out, or taken from the row above, moves dV_j by about |dO_j|.
    The merged outputs of both entries (rot_dim 64) are held to kernel_compare.merged_backward_reference from the same reference:
    the only kernel-level check of dqkv at S = 2048, the training length."""
    from magma_amd import ops
    B, H = 1, 2
    d = H * 256
    if inputs == "tile edges":
        q = rnd(B, H, S, 256, dev=dev, seed=24, scale=0.5).to(BF16)
        k = kcmp.dominant_edge_keys(q, rnd(B, H, S, 256, dev=dev, seed=25, scale=0.5).to(BF16))
        v = rnd(B, H, S, 256, dev=dev, seed=26).to(BF16)
    else:
        q, k, v = kcmp.self_dominant_qkv((B, H, S, 256), float(inputs[-1]), seed=27, device=dev)
    dO = rnd(B * S, d, dev=dev, seed=28).to(BF16)
    x = ops.AttnRows.of_bhsd(q, k, v)
    out = torch.empty(B * S, d, dtype=BF16, device=dev)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
    ops.attn_fwd_rows(x, out, lse=lse)
    kcmp.assert_causal_attention(out, q, k, v, f"attn_fwd_rows, {inputs}, S={S}", lse=lse)
    ref = kcmp.assert_attention_backward(*ops.attn_bwd_rows(x, dO, out, lse), q, k, v, dO, out, lse, f"attn_bwd_rows, {inputs}, S={S}")
    # the merged output (dqkv with the inverse rotary in the epilogue: what the training engine consumes), from the same reference
    rot = 64
    sin_t, cos_t = rot_tables(S + 3, rot, dev)
    kcmp.assert_merged_attention_backward(ops.attn_bwd_rows(x, dO, out, lse, merged_rot=(rot, sin_t, cos_t)), q, k, v, dO, out, lse,
                                          rot, sin_t, cos_t, f"attn_bwd_rows merged, {inputs}, S={S}", ref=ref)
    del ref
    hs = H * S * 256
    vt, qt, kt = (ops.head_transpose(t, B, H, S, sb=hs, ss=256, sh=S * 256) for t in (v, q, k))
    dOt = ops.head_transpose(dO, B, H, S, sb=S * d, ss=d, sh=256)
    out2, lse2 = torch.empty_like(out), torch.empty_like(lse)
    ops.attn_prefill(q, k, vt, out2, B, H, S, lse=lse2)
    ref = kcmp.assert_attention_backward(*ops.attn_bwd(q, k, v, qt, kt, dO, dOt, out2, lse2, B, H, S), q, k, v, dO, out2, lse2,
                                         f"attn_bwd, {inputs}, S={S}")
    kcmp.assert_merged_attention_backward(ops.attn_bwd_merged(q, k, v, qt, kt, dO, out2, lse2, B, H, S, rot, sin_t, cos_t), q, k, v, dO,
                                          out2, lse2, rot, sin_t, cos_t, f"attn_bwd_merged, {inputs}, S={S}", ref=ref)


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("B,H,S", [(1, 1, 1), (2, 2, 57), (1, 2, 300), (2, 1, 385), (1, 1, 1024)])
def test_attention_backward_kernel_variants(dev, monkeypatch, variant, B, H, S):
    """MAGMA_ATTN_BWD = 0 (three 16-row-wave kernels) / 1, 2 (dK and dV in one 32-key-wave kernel, S and dP computed once)
    / 3, 4 (32-query-wave dQ as well): each against fp32 autograd of the same attention, separate [B,H,S,256] outputs and
    the merged dqkv output with the inverse rotary (whole-row stores through the LDS staging image)."""
    from magma_amd import ops
    monkeypatch.setenv("MAGMA_ATTN_BWD", str(variant))
    d = H * 256
    q = rnd(B, H, S, 256, dev=dev, seed=50, scale=0.5).to(BF16)
    k = rnd(B, H, S, 256, dev=dev, seed=51, scale=0.5).to(BF16)
    v = rnd(B, H, S, 256, dev=dev, seed=52).to(BF16)
    dO = rnd(B * S, d, dev=dev, seed=53).to(BF16)
    vt = ops.head_transpose(v, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    out = torch.empty(B * S, d, dtype=BF16, device=dev)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
    ops.attn_prefill(q, k, vt, out, B, H, S, lse=lse)
    qt = ops.head_transpose(q, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    kt = ops.head_transpose(k, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    dOt = ops.head_transpose(dO, B, H, S, sb=S * d, ss=d, sh=256)
    dq, dk, dv = ops.attn_bwd(q, k, v, qt, kt, dO, dOt, out, lse, B, H, S)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    sc = qf @ kf.transpose(-1, -2) / 16.0
    sc = sc.masked_fill(~torch.ones(S, S, dtype=torch.bool, device=dev).tril(), float("-inf"))
    o = (torch.softmax(sc, -1) @ vf).permute(0, 2, 1, 3).reshape(B * S, d)
    o.backward(dO.float())
    for got, ref, name in ((dq, qf.grad, "dq"), (dk, kf.grad, "dk"), (dv, vf.grad, "dv")):
        if float(ref.abs().max()) < 1e-6:      # S = 1: softmax over one key has zero gradient
            assert float(got.float().abs().max()) < 1e-6, name
        else:
            assert rel(got, ref) < 1.5e-2, (variant, name, rel(got, ref))
    ref = kcmp.assert_attention_backward(dq, dk, dv, q, k, v, dO, out, lse, f"attn_bwd variant {variant} B={B} H={H} S={S}")
    rot = 64
    inv = 1.0 / (10000 ** (torch.arange(0, rot, 2, dtype=torch.float32, device=dev) / rot))
    ang = torch.arange(S + 3, dtype=torch.float32, device=dev)[:, None] * inv[None, :]
    sin_t, cos_t = ang.sin().contiguous(), ang.cos().contiguous()
    two_pass = ops.rotary_merge_bwd(dq, dk, dv, B, S, H, rot, sin_t, cos_t)
    merged = ops.attn_bwd_merged(q, k, v, qt, kt, dO, out, lse, B, H, S, rot, sin_t, cos_t)
    # every element of dqkv against the fp64 reference turned by the table row of its position, one rounding; the norms below stay
    # as the coarser second check
    kcmp.assert_merged_attention_backward(merged, q, k, v, dO, out, lse, rot, sin_t, cos_t,
                                          f"attn_bwd_merged variant {variant} B={B} H={H} S={S}", ref=ref)
    assert torch.equal(merged[:, 2 * d:], two_pass[:, 2 * d:])                     # dv: no rotary, same rounding
    if S > 1:
        for sl in (slice(0, d), slice(d, 2 * d)):
            assert rel(merged[:, sl], two_pass[:, sl]) < 6e-3


@pytest.mark.parametrize("B,H,S", [(2, 2, 57), (1, 2, 300)])
def test_attention_backward_merged_output(dev, B, H, S):
    """mg_attn_bwd_merged_bf16 (gradients written straight into dqkv with the inverse rotary) == mg_attn_bwd_bf16 +
    mg_rotary_merge_bwd_bf16, up to the second bf16 rounding the two-pass form has."""
    from magma_amd import ops
    d = H * 256
    q = rnd(B, H, S, 256, dev=dev, seed=30, scale=0.5).to(BF16)
    k = rnd(B, H, S, 256, dev=dev, seed=31, scale=0.5).to(BF16)
    v = rnd(B, H, S, 256, dev=dev, seed=32).to(BF16)
    dO = rnd(B * S, d, dev=dev, seed=33).to(BF16)
    vt = ops.head_transpose(v, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    out = torch.empty(B * S, d, dtype=BF16, device=dev)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
    ops.attn_prefill(q, k, vt, out, B, H, S, lse=lse)
    qt = ops.head_transpose(q, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    kt = ops.head_transpose(k, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    dOt = ops.head_transpose(dO, B, H, S, sb=S * d, ss=d, sh=256)
    rot = 64
    inv = 1.0 / (10000 ** (torch.arange(0, rot, 2, dtype=torch.float32, device=dev) / rot))
    ang = torch.arange(S + 3, dtype=torch.float32, device=dev)[:, None] * inv[None, :]
    sin_t, cos_t = ang.sin().contiguous(), ang.cos().contiguous()
    dq, dk, dv = ops.attn_bwd(q, k, v, qt, kt, dO, dOt, out, lse, B, H, S)
    two_pass = ops.rotary_merge_bwd(dq, dk, dv, B, S, H, rot, sin_t, cos_t)
    merged = ops.attn_bwd_merged(q, k, v, qt, kt, dO, out, lse, B, H, S, rot, sin_t, cos_t)   # transposes dO itself
    assert merged.shape == two_pass.shape == (B * S, 3 * d)
    assert torch.equal(merged[:, 2 * d:], two_pass[:, 2 * d:])                     # dv: no rotary, same rounding
    for name, sl in (("dq", slice(0, d)), ("dk", slice(d, 2 * d))):
        a, b = merged[:, sl].view(B * S, H, 256), two_pass[:, sl].view(B * S, H, 256)
        # columns outside the rotary: same arithmetic except the summation order of D = rowsum(dO o O) (fused prep)
        assert rel(a[..., rot:], b[..., rot:]) < 2e-3, (name, rel(a[..., rot:], b[..., rot:]))
        assert rel(a[..., :rot], b[..., :rot]) < 6e-3, (name, rel(a[..., :rot], b[..., :rot]))
    # O at the row stride of a wider buffer (the [ctx | t] operand of the training step's [W_out | W_up] GEMM): bit-identical
    wide = torch.full((B * S, d + 136), float("nan"), dtype=BF16, device=dev)
    wide[:, :d] = out
    assert torch.equal(ops.attn_bwd_merged(q, k, v, qt, kt, dO, wide[:, :d], lse, B, H, S, rot, sin_t, cos_t), merged)
    for got, ref in zip(ops.attn_bwd(q, k, v, qt, kt, dO, dOt, wide[:, :d], lse, B, H, S), (dq, dk, dv)):
        assert torch.equal(got, ref)


def test_rotary_split_train_emits_all_transposes(dev):
    """mg_rotary_split_train_bf16 == mg_rotary_split_bf16 + two mg_head_transpose_bf16, bit for bit."""
    from magma_amd import ops
    B, H, S, rot = 2, 3, 75, 64
    d = H * 256
    qkv = rnd(B * S, 3 * d, dev=dev, seed=40).to(BF16)
    inv = 1.0 / (10000 ** (torch.arange(0, rot, 2, dtype=torch.float32, device=dev) / rot))
    ang = torch.arange(S + 5, dtype=torch.float32, device=dev)[:, None] * inv[None, :]
    sin_t, cos_t = ang.sin().contiguous(), ang.cos().contiguous()
    ld = ops.ceil_to(S, 32)
    mk = lambda: torch.empty(B, H, S, 256, dtype=BF16, device=dev)
    mt = lambda: torch.full((B, H, ld // 32, 256, 32), 7.0, dtype=BF16, device=dev)
    q0, k0, v0, vt0 = mk(), mk(), mk(), mt()
    ops.rotary_split(qkv, B, S, H, rot, sin_t, cos_t, q0, k0, v0, pos0=0, vt=vt0)
    qt0 = ops.head_transpose(q0, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    kt0 = ops.head_transpose(k0, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    q1, k1, v1, vt1, qt1, kt1 = mk(), mk(), mk(), mt(), mt(), mt()
    ops.rotary_split_train(qkv, B, S, H, rot, sin_t, cos_t, q1, k1, v1, vt1, qt1, kt1)
    for a, b, name in ((q1, q0, "q"), (k1, k0, "k"), (v1, v0, "v"), (vt1, vt0, "vt"), (qt1, qt0, "qt"), (kt1, kt0, "kt")):
        assert torch.equal(a, b), name


def test_rotary_qk_inplace_equals_the_split_pass(dev):
    """mg_rotary_qk_inplace_bf16 leaves in the q / k sections of qkv exactly what mg_rotary_split_bf16 writes to q / kcache (same
    fp32 arithmetic, one bf16 rounding), v untouched; also at a row stride wider than 3 H 256."""
    from magma_amd import ops
    B, H, S, rot = 2, 3, 75, 64
    d = H * 256
    wide = rnd(B * S, 3 * d + 40, dev=dev, seed=41).to(BF16)
    qkv = wide[:, :3 * d]
    inv = 1.0 / (10000 ** (torch.arange(0, rot, 2, dtype=torch.float32, device=dev) / rot))
    ang = torch.arange(S + 5, dtype=torch.float32, device=dev)[:, None] * inv[None, :]
    sin_t, cos_t = ang.sin().contiguous(), ang.cos().contiguous()
    mk = lambda: torch.empty(B, H, S, 256, dtype=BF16, device=dev)
    q0, k0, v0 = mk(), mk(), mk()
    ops.rotary_split(qkv, B, S, H, rot, sin_t, cos_t, q0, k0, v0, pos0=0)
    before = wide.clone()
    ops.rotary_qk_inplace(qkv, B, S, H, rot, sin_t, cos_t)
    got = qkv.reshape(B, S, 3, H, 256).permute(2, 0, 3, 1, 4)
    assert torch.equal(got[0], q0) and torch.equal(got[1], k0) and torch.equal(got[2], v0)
    assert torch.equal(wide[:, 3 * d:], before[:, 3 * d:]) and torch.equal(wide[:, 2 * d:3 * d], before[:, 2 * d:3 * d])


@pytest.mark.parametrize("B,H,S", [(1, 1, 1), (2, 2, 57), (1, 2, 300), (2, 1, 385), (1, 1, 1024), (1, 3, 129)])
def test_attention_without_transposed_images(dev, B, H, S):
    """mg_attn_fwd_rows_bf16 / mg_attn_bwd_rows_bf16 (csrc/attention_tr.hip: V^T, Q^T, dO^T, K^T fragments read from the ROW images
    with ds_read_b64_tr_b16): forward and all three gradients against fp32 autograd of the same attention; against the kernels with
    transposed images (same MFMA order: the outputs agree to the last bit or nearly); and reading q / k / v straight from the fused qkv
    activation [B*S, 3 H 256] gives the SAME bits as reading [B,H,S,256] tensors -- separate and merged (inverse rotary) outputs."""
    from magma_amd import ops
    d = H * 256
    q = rnd(B, H, S, 256, dev=dev, seed=60, scale=0.5).to(BF16)
    k = rnd(B, H, S, 256, dev=dev, seed=61, scale=0.5).to(BF16)
    v = rnd(B, H, S, 256, dev=dev, seed=62).to(BF16)
    dO = rnd(B * S, d, dev=dev, seed=63).to(BF16)
    x = ops.AttnRows.of_bhsd(q, k, v)
    out = torch.empty(B * S, d, dtype=BF16, device=dev)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
    ops.attn_fwd_rows(x, out, lse=lse)
    # the same operands as column ranges of one fused activation (what the training engine hands over), wider row stride
    fused = torch.zeros(B * S, 3 * d + 24, dtype=BF16, device=dev)
    fused[:, :3 * d] = torch.stack((q, k, v)).permute(1, 3, 0, 2, 4).reshape(B * S, 3 * d)
    xf = ops.AttnRows.of_qkv(fused[:, :3 * d], B, S, H)
    out_f = torch.full((B * S, d + 8), float("nan"), dtype=BF16, device=dev)
    lse_f = torch.empty_like(lse)
    ops.attn_fwd_rows(xf, out_f[:, :d], lse=lse_f)
    assert torch.equal(out_f[:, :d], out) and torch.equal(lse_f, lse)
    # the kernels with transposed images
    vt = ops.head_transpose(v, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    out_old = torch.empty_like(out)
    lse_old = torch.empty_like(lse)
    ops.attn_prefill(q, k, vt, out_old, B, H, S, lse=lse_old)
    assert rel(out, out_old) < 1e-3 and float((lse - lse_old).abs().max()) < 1e-4
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    sc = qf @ kf.transpose(-1, -2) / 16.0
    sc = sc.masked_fill(~torch.ones(S, S, dtype=torch.bool, device=dev).tril(), float("-inf"))
    o = (torch.softmax(sc, -1) @ vf).permute(0, 2, 1, 3).reshape(B * S, d)
    assert rel(out, o.detach()) < 1e-2
    kcmp.assert_causal_attention(out, q, k, v, f"attn_fwd_rows B={B} H={H} S={S}", lse=lse)
    o.backward(dO.float())
    dq, dk, dv = ops.attn_bwd_rows(x, dO, out, lse)
    for got, ref, name in ((dq, qf.grad, "dq"), (dk, kf.grad, "dk"), (dv, vf.grad, "dv")):
        if float(ref.abs().max()) < 1e-6:      # S = 1: softmax over one key has zero gradient
            assert float(got.float().abs().max()) < 1e-6, name
        else:
            assert rel(got, ref) < 1.5e-2, (name, rel(got, ref))
    ref = kcmp.assert_attention_backward(dq, dk, dv, q, k, v, dO, out, lse, f"attn_bwd_rows B={B} H={H} S={S}")
    for a, b_ in zip(ops.attn_bwd_rows(xf, dO, out_f[:, :d], lse), (dq, dk, dv)):
        assert torch.equal(a, b_)
    rot = 64
    inv = 1.0 / (10000 ** (torch.arange(0, rot, 2, dtype=torch.float32, device=dev) / rot))
    ang = torch.arange(S + 3, dtype=torch.float32, device=dev)[:, None] * inv[None, :]
    sin_t, cos_t = ang.sin().contiguous(), ang.cos().contiguous()
    two_pass = ops.rotary_merge_bwd(dq, dk, dv, B, S, H, rot, sin_t, cos_t)
    merged = ops.attn_bwd_rows(xf, dO, out, lse, merged_rot=(rot, sin_t, cos_t))
    # dqkv per element, from both operand forms: every bit comparison below (mx_out, no_out, first_rows) rests on this tensor
    for got, form in ((merged, "fused qkv operand"), (ops.attn_bwd_rows(x, dO, out, lse, merged_rot=(rot, sin_t, cos_t)), "[B,H,S,256] operands")):
        kcmp.assert_merged_attention_backward(got, q, k, v, dO, out, lse, rot, sin_t, cos_t,
                                              f"attn_bwd_rows merged, {form}, B={B} H={H} S={S}", ref=ref)
    del ref
    assert merged.shape == (B * S, 3 * d) and torch.equal(merged[:, 2 * d:], two_pass[:, 2 * d:])
    if S > 1:
        for sl in (slice(0, d), slice(d, 2 * d)):
            assert rel(merged[:, sl], two_pass[:, sl]) < 6e-3
    # BASELINE config[4]: the epilogues' OCP MX e4m3 copy of dqkv (operand of the qkv dgrad's MX GEMM) == mg_quantize_mx_fp8(dqkv) bit
    # for bit, next to the bf16 output and on its own (no_out)
    mx = ops.mx_empty(B * S, 3 * d, dev)
    merged_b = ops.attn_bwd_rows(xf, dO, out, lse, merged_rot=(rot, sin_t, cos_t), mx_out=mx)
    qref, sref = ops.quantize_mx_fp8(merged)
    assert torch.equal(merged_b, merged) and torch.equal(mx[0], qref) and torch.equal(mx[1], sref)
    mx2 = ops.mx_empty(B * S, 3 * d, dev)
    assert ops.attn_bwd_rows(xf, dO, out, lse, merged_rot=(rot, sin_t, cos_t), mx_out=mx2, no_out=True) is None
    assert torch.equal(mx2[0], qref) and torch.equal(mx2[1], sref)
    # first_rows (the bottom block of a frozen LM: only the first positions' gradients are wanted): the first ceil(P / 128) query /
    # key blocks carry the same bits as the full launch -- dK / dV of those keys still sum over EVERY later query
    for P in (1, 49, 144, 200):
        if P >= S:
            continue
        n = min(S, (P + 127) // 128 * 128)
        for a, b_ in zip(ops.attn_bwd_rows(x, dO, out, lse, first_rows=P), (dq, dk, dv)):
            assert torch.equal(a[:, :, :n], b_[:, :, :n]), P
        part = ops.attn_bwd_rows(xf, dO, out, lse, merged_rot=(rot, sin_t, cos_t), first_rows=P)
        assert torch.equal(part.view(B, S, 3 * d)[:, :n], merged.view(B, S, 3 * d)[:, :n]), P


def merged_sections(dqkv, B, H, S):
    """dqkv [B*S, 3 H 256] -> its dq, dk, dv sections as [B, H, S, 256] views (grad_row_ptr, csrc/attn_bwd_device.h)."""
    x = dqkv.view(B, S, 3, H, 256).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


MERGED_S_LADDER = (1, 31, 32, 33, 127, 128, 129, 257)        # around the 32-row wave tiles and the 128-row blocks
MERGED_ROT_LADDER = (0, 8, 32, 256)                          # at S = 129; rot_dim 64 is the S ladder's


@pytest.mark.parametrize("inputs", kcmp.MERGED_BWD_FAMILIES)
@pytest.mark.parametrize("S,rot", [(S, 64) for S in MERGED_S_LADDER] + [(129, r) for r in MERGED_ROT_LADDER])
def test_merged_backward_sequence_and_rotary_edges(dev, monkeypatch, S, rot, inputs):
    """dqkv of the rows entry (mg_attn_bwd_rows_bf16) and of mg_attn_bwd_merged_bf16 at one variant per epilogue -- 0: store_grad_row,
    3: store_grad_tile32, 8: store_grad_tile32_tr -- per element against kernel_compare.merged_backward_reference, B = 2, H = 2:
    with a ragged S the rows a tile holds past S lie next to the NEXT batch item's rows, and the tables [S + 3, rot / 2] have rows
    past S that a position off by one would read.  Inputs: kernel_compare.merged_backward_inputs (for which the CPU suite shows
    every single-row fault of an epilogue at 8 bounds and more).  dqkv is handed over full of NaN: every element must be written.
    Where the merged and the separate form issue the SAME launches -- the rows entry, and variant 8 (>= 5: attn_bwd_prep_kernel
    in both) -- the columns the rotary does not touch (all of them at rot_dim 0, all of dv always) agree bit for bit with the
    separate dq / dk / dv.  Variants 0 and 3 take D = rowsum(dO o O) from attn_bwd_prep_t_kernel in the merged form, another
    summation order: there dq and dk have the per-element bound only, and dv (which does not depend on D) the bits."""
    from magma_amd import ops
    B, H = 2, 2
    d = H * 256
    q, k, v, dO = (t.to(dev) for t in kcmp.merged_backward_inputs(inputs, B, H, S))
    x = ops.AttnRows.of_bhsd(q, k, v)
    out = torch.empty(B * S, d, dtype=BF16, device=dev)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
    ops.attn_fwd_rows(x, out, lse=lse)
    sin_t, cos_t = rot_tables(S + 3, rot, dev)
    ref = kcmp.attention_backward_reference(q, k, v, dO, out, lse)
    hs = H * S * 256
    qt, kt = (ops.head_transpose(t, B, H, S, sb=hs, ss=256, sh=S * 256) for t in (q, k))
    dOt = ops.head_transpose(dO, B, H, S, sb=S * d, ss=d, sh=256)

    def check(dqkv, sep, what, same_launches):
        assert bool(torch.isfinite(dqkv).all()), f"{what}: {int((~torch.isfinite(dqkv)).sum())} elements of dqkv not written"
        kcmp.assert_merged_attention_backward(dqkv, q, k, v, dO, out, lse, rot, sin_t, cos_t, f"{what}, {inputs}, S={S} rot={rot}", ref=ref)
        mq, mk, mv = merged_sections(dqkv, B, H, S)
        assert torch.equal(mv, sep[2]), f"{what}: dv"
        if same_launches:
            assert torch.equal(mq[..., rot:], sep[0][..., rot:]) and torch.equal(mk[..., rot:], sep[1][..., rot:]), f"{what}: columns >= rot_dim"

    nan = lambda: torch.full((B * S, 3 * d), float("nan"), dtype=BF16, device=dev)
    check(ops.attn_bwd_rows(x, dO, out, lse, merged_rot=(rot, sin_t, cos_t), out=nan()), ops.attn_bwd_rows(x, dO, out, lse), "attn_bwd_rows merged", True)
    for variant in (0, 3, 8):
        monkeypatch.setenv("MAGMA_ATTN_BWD", str(variant))
        sep = ops.attn_bwd(q, k, v, qt, kt, dO, dOt, out, lse, B, H, S)
        dqkv = ops.attn_bwd_merged(q, k, v, qt, kt, dO, out, lse, B, H, S, rot, sin_t, cos_t, out=nan())
        check(dqkv, sep, f"attn_bwd_merged variant {variant}", variant >= 5)


SENTINEL = -1232.0          # exact in bf16; nothing the kernels compute from these inputs comes near it


@pytest.mark.parametrize("P", [1, 127, 128, 129])
def test_attention_backward_first_rows_leaves_the_rest_unwritten(dev, P):
    """first_rows = P at S = 300 (B = 2, H = 2): the first ceil(P / 128) blocks of 128 positions carry the bits of the full launch --
    whose merged output is held to the per-element bound here -- and every row from ceil(P / 128) 128 on still holds what the
    caller put there, in the merged and in the separate form: a block too many, or a tile that runs past its block, shows."""
    from magma_amd import ops
    B, H, S, rot = 2, 2, 300, 64
    d = H * 256
    q, k, v, dO = (t.to(dev) for t in kcmp.merged_backward_inputs("i.i.d.", B, H, S))
    x = ops.AttnRows.of_bhsd(q, k, v)
    out = torch.empty(B * S, d, dtype=BF16, device=dev)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
    ops.attn_fwd_rows(x, out, lse=lse)
    sin_t, cos_t = rot_tables(S + 3, rot, dev)
    full_sep = ops.attn_bwd_rows(x, dO, out, lse)
    full = ops.attn_bwd_rows(x, dO, out, lse, merged_rot=(rot, sin_t, cos_t))
    ref = kcmp.assert_attention_backward(*full_sep, q, k, v, dO, out, lse, "attn_bwd_rows (full launch of the first_rows test)")
    kcmp.assert_merged_attention_backward(full, q, k, v, dO, out, lse, rot, sin_t, cos_t, "attn_bwd_rows merged (full launch)", ref=ref)
    n = (P + 127) // 128 * 128
    assert n < S
    part = ops.attn_bwd_rows(x, dO, out, lse, merged_rot=(rot, sin_t, cos_t), first_rows=P,
                             out=torch.full((B * S, 3 * d), SENTINEL, dtype=BF16, device=dev)).view(B, S, 3 * d)
    assert torch.equal(part[:, :n], full.view(B, S, 3 * d)[:, :n]), "merged: the written rows"
    assert bool((part[:, n:] == SENTINEL).all()), f"merged: {int((part[:, n:] != SENTINEL).sum())} elements written at positions >= {n}"
    outs = tuple(torch.full((B, H, S, 256), SENTINEL, dtype=BF16, device=dev) for _ in range(3))
    for got, want, name in zip(ops.attn_bwd_rows(x, dO, out, lse, first_rows=P, out=outs), full_sep, ("dq", "dk", "dv")):
        assert torch.equal(got[:, :, :n], want[:, :, :n]), f"{name}: the written rows"
        assert bool((got[:, :, n:] == SENTINEL).all()), f"{name}: {int((got[:, :, n:] != SENTINEL).sum())} elements written at positions >= {n}"


def test_rotary_merge_bwd(dev):
    from magma_amd import ops
    from oracle.model import apply_rotary, rotary_tables
    B, S, H = 2, 37, 2
    sin_t, cos_t = rotary_tables(64, 64)
    dq, dk, dv = (rnd(B, H, S, 256, dev=dev, seed=30 + i).to(BF16) for i in range(3))
    out = ops.rotary_merge_bwd(dq, dk, dv, B, S, H, 64, sin_t.to(dev).contiguous(), cos_t.to(dev).contiguous())
    x = torch.zeros(B, S, H, 256, requires_grad=True)
    y = apply_rotary(x, torch.arange(S), 64)
    y.backward(dq.float().cpu().permute(0, 2, 1, 3))
    got = out.view(B, S, 3, H, 256).float().cpu()
    assert rel(got[:, :, 0], x.grad) < 4e-3
    assert torch.equal(got[:, :, 2], dv.float().cpu().permute(0, 2, 1, 3))
    # per element: the inverse rotation R(-theta) of dq and dk = the rotary with -sin
    sd, cd = sin_t[:S].to(dev)[:, None, :], cos_t[:S].to(dev)[:, None, :]
    gd = out.view(B, S, 3, H, 256)
    for i, (src, name) in enumerate(((dq, "dq"), (dk, "dk"))):
        rref, rbound = kcmp.rotary_reference(src.permute(0, 2, 1, 3), -sd, cd, 64)
        kcmp.assert_elementwise(gd[:, :, i], rref, rbound, f"rotary_merge_bwd {name}")


def test_conv_backward_helpers(dev):
    from magma_amd import ops
    B, H, W, C = 2, 6, 8, 16
    dy = rnd(B, H // 2, W // 2, C, dev=dev, seed=40).to(BF16)
    dx = ops.avgpool2_bwd(dy, B, H, W, C)
    xr = torch.zeros(B, C, H, W, device=dev, requires_grad=True)
    F.avg_pool2d(xr, 2).backward(dy.float().permute(0, 3, 1, 2))
    assert rel(dx, xr.grad.permute(0, 2, 3, 1)) < 4e-3
    dx_ref = (dy.double() / 4).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)      # each input pixel gets dy / 4
    kcmp.assert_elementwise(dx, dx_ref, kcmp.map_bound(dx_ref, dx_ref.abs(), 1, BF16), "avgpool2_bwd")
    a, b, gt = (rnd(64, 24, dev=dev, seed=41 + i).to(BF16) for i in range(3))
    assert rel(ops.add_gate(a, b, gt), (a.float() + b.float()) * (gt.float() > 0)) < 4e-3
    ag_ref = (a.double() + b.double()) * (gt.double() > 0)
    kcmp.assert_elementwise(ops.add_gate(a, b, gt), ag_ref, kcmp.map_bound(ag_ref, (a.double().abs() + b.double().abs()) * (gt.double() > 0), 1, BF16),
                            "add_gate")
    assert torch.equal(ops.add_gate(a), a)
    # im2col^T x dY^T == conv weight gradient
    x = rnd(B, H, W, C, dev=dev, seed=44).to(BF16)
    cols_t = ops.im2col_t(x, B, H, W, C)
    ref = F.unfold(x.float().permute(0, 3, 1, 2), 3, padding=1)          # [B, C*9, HW], row = c*9 + tap
    ref = ref.permute(1, 0, 2).reshape(9 * C, B * H * W)
    assert torch.equal(cols_t.float()[:, : B * H * W], ref)
    # frozen-stat BN affine grads
    M = B * H * W
    g = rnd(M, C, dev=dev, seed=45).to(BF16)
    y = rnd(M, C, dev=dev, seed=46).to(BF16)
    sub = rnd(M, C, dev=dev, seed=47).to(BF16)
    gamma, beta = rnd(C, dev=dev, seed=48) + 2, rnd(C, dev=dev, seed=49)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    ops.bn_param_grad(g, y, sub, gamma, beta, dg, db)
    assert rel(db, g.float().sum(0)) < 1e-4
    assert rel(dg, (g.float() * (y.float() - sub.float() - beta) / gamma).sum(0)) < 1e-4
    g64, y64, s64 = g.double(), y.double(), sub.double()
    db_r, dg_r = g64.sum(0), (g64 * (y64 - s64 - beta.double()) / gamma.double()).sum(0)
    dg_m = (g64.abs() * (y64.abs() + s64.abs() + beta.double().abs()) / gamma.double().abs()).sum(0)
    kcmp.assert_elementwise(db, db_r, kcmp.rounded(db_r, kcmp.gamma(M + 8) * g64.abs().sum(0), torch.float32), f"bn_param_grad dbeta {M}x{C}")
    kcmp.assert_elementwise(dg, dg_r, kcmp.rounded(dg_r, kcmp.gamma(M + 12) * dg_m, torch.float32), f"bn_param_grad dgamma {M}x{C}")
    # ragged row counts around the kernel's 16-row groups / 256-row blocks, with and without the residual operand, C > 512
    for M2, C2, with_sub in ((1, 8, True), (267, 520, False), (513 + 7, 40, True)):
        g2, y2 = rnd(M2, C2, dev=dev, seed=52).to(BF16), rnd(M2, C2, dev=dev, seed=53).to(BF16)
        s2 = rnd(M2, C2, dev=dev, seed=54).to(BF16) if with_sub else None
        gm, bt = rnd(C2, dev=dev, seed=55) + 2, rnd(C2, dev=dev, seed=56)
        dg2, db2 = torch.zeros(C2, device=dev), torch.zeros(C2, device=dev)
        ops.bn_param_grad(g2, y2, s2, gm, bt, dg2, db2)
        yy = y2.float() - (s2.float() if with_sub else 0)
        assert rel(db2, g2.float().sum(0)) < 1e-4 and rel(dg2, (g2.float() * (yy - bt) / gm).sum(0)) < 1e-4, (M2, C2)
        # per element: column sums over M2 rows in fp32 (any order: threads, LDS, atomics), four operations per term of dgamma
        y64 = y2.double() - (s2.double() if with_sub else 0.0)
        db_r, db_m = g2.double().sum(0), g2.double().abs().sum(0)
        dg_r = (g2.double() * (y64 - bt.double()) / gm.double()).sum(0)
        dg_m = (g2.double().abs() * (y2.double().abs() + (s2.double().abs() if with_sub else 0.0) + bt.double().abs()) / gm.double().abs()).sum(0)
        kcmp.assert_elementwise(db2, db_r, kcmp.rounded(db_r, kcmp.gamma(M2 + 8) * db_m, torch.float32), f"bn_param_grad dbeta {M2}x{C2}")
        kcmp.assert_elementwise(dg2, dg_r, kcmp.rounded(dg_r, kcmp.gamma(M2 + 12) * dg_m, torch.float32), f"bn_param_grad dgamma {M2}x{C2}")
        # the same sums taken while g is transposed for the weight-gradient GEMM (one pass over g): the transpose bit for bit, the
        # sums accumulated ON TOP of what the buffers hold
        dg3, db3 = torch.full((C2,), 3.0, device=dev), torch.full((C2,), -2.0, device=dev)
        gt = ops.transpose_bn_param_grad(g2, y2, s2, gm, bt, dg3, db3)
        assert torch.equal(gt, ops.transpose(g2))
        assert rel(db3 + 2.0, g2.float().sum(0)) < 1e-4 and rel(dg3 - 3.0, (g2.float() * (yy - bt) / gm).sum(0)) < 1e-4, (M2, C2)


def test_adamw_and_clip(dev):
    from magma_amd import ops
    n = 10007
    p0 = rnd(n, dev=dev, seed=50)
    g = rnd(n, dev=dev, seed=51) * 3
    ref_p = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref_p], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    p, m, v = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pb = torch.empty(n, dtype=BF16, device=dev)
    for step in (1, 2, 3):
        ref_p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([ref_p], 1.0)
        opt.step()
        nsq = torch.zeros(1, device=dev)
        ops.sumsq(g, nsq)
        before = (p.clone(), m.clone(), v.clone())
        ops.adamw(p, m, v, g, pb, 1e-2, 0.9, 0.95, 1e-8, 0.1, step, max_norm=1.0, norm_sq=nsq)
        # per element, each step from the state the kernel itself left (errors of earlier steps are not re-counted)
        R = kcmp.adamw_reference(*before, g, nsq, 1e-2, 0.9, 0.95, 1e-8, 0.1, step, 1.0)
        for name, got in (("m", m), ("v", v), ("p", p), ("p_bf16", pb)):
            kcmp.assert_elementwise(got, *R[name], f"adamw + clip, step {step}, {name}")
    assert rel(p, ref_p.detach()) < 1e-5
    assert torch.equal(pb, p.to(BF16))


@pytest.mark.parametrize("cout,cin,k", [(24, 16, 3), (96, 48, 3), (40, 72, 1), (768, 768, 3)])
def test_conv_weight_relayout(dev, cout, cin, k):
    """bit-exact against the PyTorch expressions it replaces in the training engine"""
    from magma_amd import ops
    w = rnd(cout, cin, k, k, dev=dev, seed=50, scale=0.1).to(BF16)
    scale = rnd(cout, dev=dev, seed=51).abs() + 0.5
    f = ops.conv_weight_relayout(w, 0)
    ref_f = w.permute(0, 2, 3, 1).reshape(cout, k * k * cin)
    assert f.shape[1] % 64 == 0 and torch.equal(f[:, : k * k * cin], ref_f) and bool((f[:, k * k * cin:] == 0).all())
    d = ops.conv_weight_relayout(w, 1, scale)
    ref_d = (w.float() * scale.view(cout, 1, 1, 1)).flip(2, 3).permute(1, 2, 3, 0).reshape(cin, k * k * cout).to(BF16)
    assert d.shape[1] % 64 == 0 and torch.equal(d[:, : k * k * cout], ref_d) and bool((d[:, k * k * cout:] == 0).all())


def test_conv_operand_plan_matches_the_single_calls(dev):
    """mg_conv_weight_relayout_batch / mg_bn_fold_batch (ops.ConvOperandPlan: every convolution of the CLIP trunk re-derived by two
    launches per step) == mg_conv_weight_relayout_bf16 / mg_bn_fold_f32 per convolution, bit for bit -- 1x1 and 3x3, ragged
    channel counts, a 1x1 whose Cin is a multiple of 64 (no forward copy: the weight is its own operand); refresh() after the
    weights changed in place picks the new values up."""
    from magma_amd import ops
    shapes = [(24, 16, 3), (96, 48, 3), (40, 72, 1), (128, 64, 1), (384, 384, 3), (8, 8, 1), (3072, 768, 1)]
    units = []
    for i, (cout, cin, k) in enumerate(shapes):
        w = rnd(cout, cin, k, k, dev=dev, seed=600 + i, scale=0.1).to(BF16).contiguous()
        gamma, beta = rnd(cout, dev=dev, seed=620 + i) + 2, rnd(cout, dev=dev, seed=640 + i)
        mean, var = rnd(cout, dev=dev, seed=660 + i), rnd(cout, dev=dev, seed=680 + i).abs() + 0.1
        units.append((w, gamma.contiguous(), beta.contiguous(), mean.contiguous(), var.contiguous(), 1e-5 * (i + 1)))
    plan = ops.ConvOperandPlan(units, dev)
    for rnd_no in range(2):
        plan.refresh()
        for i, (w, gamma, beta, mean, var, eps) in enumerate(units):
            sc, sh = ops.bn_fold(gamma, beta, mean, var, eps)
            assert torch.equal(plan.scale[i], sc) and torch.equal(plan.shift[i], sh), i
            cout, cin, k, _ = w.shape
            f = ops.conv_weight_relayout(w, 0)
            if k == 1 and cin % 64 == 0:
                assert plan.fwd[i].data_ptr() == w.data_ptr() and torch.equal(plan.fwd[i], f[:, :cin])
            else:
                assert torch.equal(plan.fwd[i], f), i
            assert torch.equal(plan.dgrad[i], ops.conv_weight_relayout(w, 1, sc)), i
        for (w, gamma, *_r) in units:          # an optimizer step: same storage, new values
            w.mul_(1.5)
            gamma.add_(0.25)


@pytest.mark.parametrize("R,C", [(4096, 1024), (1000, 520), (77, 64)])
def test_transpose_colsum(dev, R, C):
    """transpose + column sums in one pass == transpose and colsum separately (bias gradient and weight-gradient operand of a Linear)."""
    from magma_amd import ops
    g = torch.Generator(device="cpu").manual_seed(R + C)
    x = torch.randn(R, C, generator=g).to(torch.bfloat16).to(dev)
    acc = torch.full((C,), 0.5, dtype=torch.float32, device=dev)           # accumulates on top of what is there
    xt = ops.transpose_colsum(x, acc)
    assert torch.equal(xt[:, :R], x.t())
    assert bool((xt[:, R:] == 0).all())
    ref = 0.5 + x.float().sum(0)
    assert float((acc - ref).abs().max()) <= 1e-3 * float(ref.abs().max()) + 1e-3
    # per element, the bound of test_colsum: R terms and the start value added in fp32 in any order (tile partials, wave
    # reductions, the atomic onto what is there), relative to the magnitude sum
    s, m = 0.5 + x.double().sum(0), 0.5 + x.double().abs().sum(0)
    kcmp.assert_elementwise(acc, s, kcmp.rounded(s, kcmp.gamma(R + 9) * m, torch.float32), f"transpose_colsum R={R} C={C}")


# ---------------------------------------------------------------------------------------------------------------------------
# entry points that only whole-model tests reached: each against an fp64 statement of the same operation, per element
# (tests/kernel_compare.py), at one aligned and one ragged shape
# ---------------------------------------------------------------------------------------------------------------------------
U32 = kcmp.U_F32


@pytest.mark.parametrize("n", [8 * 4096, 8 * 37, 8])
def test_mul(dev, n):
    """mg_mul_bf16 (dropout backward): one fp32 product rounded to bf16."""
    from magma_amd import ops
    a, b = rnd(n, dev=dev, seed=801).to(BF16), rnd(n, dev=dev, seed=802).to(BF16)
    ref = a.double() * b.double()
    kcmp.assert_elementwise(ops.mul(a, b), ref, kcmp.map_bound(ref, ref.abs(), 1, BF16), f"mul n={n}")


@pytest.mark.parametrize("rows,cols,ld", [(64, 256, 256), (37, 203, 208), (1, 5, 9)])
@pytest.mark.parametrize("with_scale", [False, True])
def test_scale_rows_acc(dev, rows, cols, ld, with_scale):
    """mg_scale_rows_acc_f32: dst[r, c] += src[r, c] * row_scale[r] in fp32, src at a row stride wider than cols; the columns of src
    past cols never reach dst."""
    from magma_amd import ops
    dst0 = rnd(rows, cols, dev=dev, seed=811)
    wide = rnd(rows, ld, dev=dev, seed=812)
    rs = rnd(rows, dev=dev, seed=813) if with_scale else None
    dst = dst0.clone()
    ops.scale_rows_acc(dst, wide[:, :cols], rs)
    term = wide[:, :cols].double() * (rs.double()[:, None] if with_scale else 1.0)
    ref = dst0.double() + term
    kcmp.assert_elementwise(dst, ref, kcmp.map_bound(ref, dst0.double().abs() + term.abs(), 2, torch.float32),
                            f"scale_rows_acc {rows}x{cols} ld {ld} row_scale={with_scale}")


@pytest.mark.parametrize("M,C,K", [(1, 8, 27), (267, 520, 72), (520, 40, 264), (64, 16, 2053)])
def test_scale_rows_acc_bn_grad(dev, M, C, K):
    """mg_scale_rows_acc_bn_grad_f32 from src = g^T a (fp32, row stride wider than K), w (bf16 [C, K]) and gsum = sum_m g:
        dst += src * row_scale[r];  dbeta += gsum;  dgamma[r] += rsqrt(var + eps) * (<src[r], w[r]> - mean[r] gsum[r]),
    ON TOP of what the three buffers hold.  Checked twice: per element against fp64 on the operands the kernel reads (a row dot of K
    fp32 products in any order, three more operations, v_rsq_f32), and -- what the entry point is for -- dgamma against the LAYER,
    sum_m g (z - mean) rstd with z = a W^T in fp64, where the bound also carries the fp32 accumulation of src over M rows.  The
    gains of this BatchNorm do not enter: the result is the same for gamma = 0 (row_scale = 0 on every fourth row here).
    Ragged shapes of test_conv_backward_helpers (M 1 / 267 / 520, C 8 / 520 / 40), K = 27 (the stem), below and above one
    256-thread sweep, and 2053 = 8 sweeps + 5."""
    from magma_amd import ops
    eps = 1e-5
    g, a = rnd(M, C, dev=dev, seed=841).to(BF16), rnd(M, K, dev=dev, seed=842).relu().to(BF16)
    w = (rnd(C, K, dev=dev, seed=843) * math.sqrt(2.0 / K)).to(BF16)
    mean, var = rnd(C, dev=dev, seed=844), torch.exp(1.5 * rnd(C, dev=dev, seed=845))
    rs = rnd(C, dev=dev, seed=846)
    rs[0::4] = 0.0
    wide = torch.full((C, K + 5), float("nan"), device=dev)
    wide[:, :K] = g.float().t() @ a.float()
    src = wide[:, :K]
    gsum = g.float().sum(0).contiguous()
    dst0, dg0, db0 = rnd(C, K, dev=dev, seed=847), rnd(C, dev=dev, seed=848), rnd(C, dev=dev, seed=849)
    dst, dg, db = dst0.clone(), dg0.clone(), db0.clone()
    ops.scale_rows_acc_bn_grad(dst, src, w, rs, mean, var, eps, gsum, dg, db)
    tag = f"scale_rows_acc_bn_grad M={M} C={C} K={K}"
    f32, s64, w64 = torch.float32, src.double(), w.double()
    term = s64 * rs.double()[:, None]
    kcmp.assert_elementwise(dst, dst0.double() + term, kcmp.map_bound(dst0.double() + term, dst0.double().abs() + term.abs(), 2, f32), tag + " dst")
    kcmp.assert_elementwise(db, db0.double() + gsum.double(), kcmp.map_bound(db0.double() + gsum.double(), db0.double().abs() + gsum.double().abs(), 1, f32),
                            tag + " dbeta")
    eps32 = float(torch.tensor(eps, dtype=f32))
    rstd = (var.double() + eps32).rsqrt()
    mg = mean.double() * gsum.double()

    def dgamma_bound(dot, dot_mag, dot_err):
        t = dot - mg
        e_t = kcmp.gamma(K + 2) * (dot_mag + mg.abs()) + dot_err                 # K products summed in any order, the product, the difference
        val = rstd * t
        e_val = rstd * e_t + val.abs() * (kcmp.U_TRANS + 3 * U32)              # var + eps, v_rsq_f32, the product
        ref = dg0.double() + val
        return ref, kcmp.rounded(ref, e_val + U32 * (dg0.double().abs() + val.abs()), f32)

    ref, bound = dgamma_bound((s64 * w64).sum(1), (s64 * w64).abs().sum(1), 0.0)
    kcmp.assert_elementwise(dg, ref, bound, tag + " dgamma (operands)")
    # the layer: z = a W^T, dgamma = sum_m g (z - mean) rstd; src carries gamma(M) |g|^T |a| of its own
    g64, a64 = g.double(), a.double()
    z = a64 @ w64.t()
    gz_mag = ((g64.abs().t() @ a64.abs()) * w64.abs()).sum(1)
    operand_err = kcmp.gamma(M) * (gz_mag + mean.double().abs() * g64.abs().sum(0))          # src and gsum: fp32 sums over M rows
    _, bound_l = dgamma_bound((g64 * z).sum(0), gz_mag, operand_err)
    ref_l = dg0.double() + (g64 * (z - mean.double()) * rstd).sum(0)
    kcmp.assert_elementwise(dg, ref_l, bound_l, tag + " dgamma (layer)")
    assert bool(torch.isnan(wide[:, K:]).all())


@pytest.mark.parametrize("n", [4 * 65536, 4 * 1001, 4])
def test_cast_f32_bf16(dev, n):
    """mg_cast_f32_bf16: round to nearest even, bit for bit what torch's cast gives -- ties to either side and a value just above
    a tie among the inputs."""
    from magma_amd import ops
    src = rnd(n, dev=dev, seed=821) * 3
    special = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, -(1 + 2.0 ** -8)], device=dev)
    src[:4] = special
    dst = torch.full((n,), float("nan"), dtype=BF16, device=dev)
    ops.cast_f32_bf16(src, dst)
    assert torch.equal(dst, src.to(BF16))


@pytest.mark.parametrize("C", [256, 300, 8])
@pytest.mark.parametrize("M", [1568, 37])
def test_bn_batch_fold(dev, C, M):
    """mg_bn_batch_fold_f32: per-channel sums -> (scale, shift, mean, rstd) and the in-place running-statistics update of
    nn.BatchNorm2d (momentum, unbiased variance), against fp64 on the same sums.  var = E[x^2] - mean^2 cancels: its bound
    is relative to E[x^2] + mean^2, and rstd inherits half of it relative to var + eps."""
    from magma_amd import ops
    eps, mom = 1e-5, 0.1
    x = rnd(M, C, dev=dev, seed=831) * (rnd(C, dev=dev, seed=832).abs() + 0.5) + rnd(C, dev=dev, seed=833) * 0.5
    s1, s2 = x.sum(0).contiguous(), (x * x).sum(0).contiguous()
    g, b = rnd(C, dev=dev, seed=834) * 0.2 + 1, rnd(C, dev=dev, seed=835) * 0.2
    rm0, rv0 = rnd(C, dev=dev, seed=836), rnd(C, dev=dev, seed=837).abs() + 0.3
    rm, rv = rm0.clone(), rv0.clone()
    scale, shift, mean, rstd = ops.bn_batch_fold(s1, s2, g, b, M, eps, mom, rm, rv)
    inv_m = 1.0 / M
    mom32, eps32 = float(torch.tensor(mom, dtype=torch.float32)), float(torch.tensor(eps, dtype=torch.float32))
    mean_r = s1.double() * inv_m
    ex2 = s2.double() * inv_m
    var_r = (ex2 - mean_r ** 2).clamp_min(0)
    rstd_r = (var_r + eps32).rsqrt()
    scale_r = g.double() * rstd_r
    shift_r = b.double() - mean_r * scale_r
    unb = M / (M - 1)
    rm_r = (1 - mom32) * rm0.double() + mom32 * mean_r
    rv_r = (1 - mom32) * rv0.double() + mom32 * var_r * unb
    d_mean = kcmp.gamma(2) * mean_r.abs()                                   # 1 / M rounded, one product
    d_var = kcmp.gamma(4) * (ex2 + mean_r ** 2) + 2 * mean_r.abs() * d_mean
    rel_rstd = 0.5 * d_var / (var_r + eps32) + kcmp.U_TRANS + 2 * U32      # v_rsq_f32 (1 ulp), the addition of eps
    f32 = torch.float32
    tag = f"bn_batch_fold C={C} M={M}"
    kcmp.assert_elementwise(mean, mean_r, kcmp.rounded(mean_r, d_mean, f32), tag + " mean")
    kcmp.assert_elementwise(rstd, rstd_r, kcmp.rounded(rstd_r, rel_rstd * rstd_r, f32), tag + " rstd")
    kcmp.assert_elementwise(scale, scale_r, kcmp.rounded(scale_r, (rel_rstd + U32) * scale_r.abs(), f32), tag + " scale")
    d_ms = (mean_r * scale_r).abs() * (kcmp.gamma(2) + rel_rstd + 2 * U32)
    kcmp.assert_elementwise(shift, shift_r, kcmp.rounded(shift_r, d_ms + U32 * (b.double().abs() + (mean_r * scale_r).abs()), f32), tag + " shift")
    run_mag = ((1 - mom32) * rm0.double()).abs() + (mom32 * mean_r).abs()
    kcmp.assert_elementwise(rm, rm_r, kcmp.rounded(rm_r, kcmp.gamma(4) * run_mag + mom32 * d_mean, f32), tag + " running mean (in place)")
    run_mag = ((1 - mom32) * rv0.double()).abs() + (mom32 * var_r * unb).abs()
    kcmp.assert_elementwise(rv, rv_r, kcmp.rounded(rv_r, kcmp.gamma(5) * run_mag + mom32 * unb * d_var, f32), tag + " running variance (in place)")
    # without running statistics nothing else changes
    out2 = ops.bn_batch_fold(s1, s2, g, b, M, eps, mom)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(out2, (scale, shift, mean, rstd)))


@pytest.mark.parametrize("M,C", [(64, 64), (37, 40), (1, 8), (4099, 264)])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_bn_apply(dev, M, C, relu, with_res):
    """mg_bn_apply_bf16: y = [relu](z * scale[c] + shift[c] [+ res]), three fp32 operations, one rounding to bf16."""
    from magma_amd import ops
    z = rnd(M, C, dev=dev, seed=841).to(BF16)
    res = rnd(M, C, dev=dev, seed=842).to(BF16) if with_res else None
    scale, shift = rnd(C, dev=dev, seed=843) * 0.3 + 1, rnd(C, dev=dev, seed=844)
    y = ops.bn_apply(z, scale, shift, res, relu)
    pre = z.double() * scale.double() + shift.double() + (res.double() if with_res else 0.0)
    mag = (z.double() * scale.double()).abs() + shift.double().abs() + (res.double().abs() if with_res else 0.0)
    ref = pre.clamp_min(0) if relu else pre
    kcmp.assert_elementwise(y, ref, kcmp.map_bound(ref, mag, 3, BF16), f"bn_apply {M}x{C} relu={relu} res={with_res}")


@pytest.mark.parametrize("M,C", [(64, 64), (37, 40), (1, 8), (4099, 264)])
def test_bn_bwd_dz(dev, M, C):
    """mg_bn_bwd_dz_bf16: dz = gamma rstd (g - dbeta / M - xhat dgamma / M), xhat = (z - mean) rstd; ten fp32 operations at most on
    the way of a term (1 / M is itself rounded), magnitudes summed without cancellation, one rounding to bf16."""
    from magma_amd import ops
    g = rnd(M, C, dev=dev, seed=851).to(BF16)
    z = (rnd(M, C, dev=dev, seed=852) * 2 + 0.3).to(BF16)
    mean, rstd = rnd(C, dev=dev, seed=853) * 0.3, rnd(C, dev=dev, seed=854).abs() * 0.3 + 0.4
    gamma_, dgamma, dbeta = rnd(C, dev=dev, seed=855) * 0.2 + 1, rnd(C, dev=dev, seed=856) * M ** 0.5, rnd(C, dev=dev, seed=857) * M ** 0.5
    dz = ops.bn_bwd_dz(g, z, mean, rstd, gamma_, dgamma, dbeta)
    d64 = lambda t: t.double()
    xh = (d64(z) - d64(mean)) * d64(rstd)
    xh_mag = (d64(z).abs() + d64(mean).abs()) * d64(rstd)
    t2, t3, t3_mag = d64(dbeta) / M, xh * d64(dgamma) / M, xh_mag * d64(dgamma).abs() / M
    k = (d64(gamma_) * d64(rstd)).abs()
    ref = d64(gamma_) * d64(rstd) * (d64(g) - t2 - t3)
    kcmp.assert_elementwise(dz, ref, kcmp.map_bound(ref, k * (d64(g).abs() + t2.abs() + t3_mag), 10, BF16), f"bn_bwd_dz {M}x{C}")


@pytest.mark.parametrize("n", [8 * 4096 + 3, 1000, 1 << 20])
def test_sumsq_bf16_gradients(dev, n):
    """mg_sumsq_bf16 (the bf16 buckets of the data-parallel step; ops.sumsq dispatches on the dtype): out[0] += sum g^2.  A term
    passes through at most n / 256 additions in its thread, 9 in the workgroup and one atomic per workgroup (<= 2048)."""
    from magma_amd import ops
    g = (rnd(n, dev=dev, seed=861) * 3).to(BF16)
    out = torch.full((1,), 2.5, device=dev)
    ops.sumsq(g, out)
    ref = 2.5 + (g.double() ** 2).sum().reshape(1)
    kcmp.assert_elementwise(out, ref, kcmp.rounded(ref, kcmp.gamma(n // 256 + 2048 + 16) * ref, torch.float32), f"sumsq bf16 n={n}")
    out32 = torch.full((1,), 2.5, device=dev)
    ops.sumsq(g.float(), out32)                         # the fp32 form on the same values
    kcmp.assert_elementwise(out32, ref, kcmp.rounded(ref, kcmp.gamma(n // 256 + 2048 + 16) * ref, torch.float32), f"sumsq f32 n={n}")


@pytest.mark.parametrize("gdtype", [BF16, torch.float32])
@pytest.mark.parametrize("n", [10007, 1 << 16, 515])
def test_adamw_one_step_per_element(dev, n, gdtype):
    """mg_adamw_gbf16_f32 / mg_adamw_f32 (ops.adamw dispatches on the gradient's dtype): ONE step from a given state (p, m, v all
    non-trivial, step 3) with clipping and a gradient scale, p / m / v / the bf16 model copy per element against fp64 on the same
    fp32 inputs and hyper-parameters.  The bias corrections 1 - beta^step cancel: their relative error is
    3 u32 beta^step / (1 - beta^step) (powf to 2 ulp, one subtraction)."""
    from magma_amd import ops
    lr, b1, b2, eps, wd, step, max_norm, gs = 1e-2, 0.9, 0.95, 1e-8, 0.1, 3, 1.0, 0.25
    p0 = rnd(n, dev=dev, seed=871)
    m0 = rnd(n, dev=dev, seed=872) * 0.1
    v0 = rnd(n, dev=dev, seed=873).abs() * 0.01
    g = (rnd(n, dev=dev, seed=874) * 3).to(gdtype)
    nsq = torch.zeros(1, device=dev)
    ops.sumsq(g, nsq)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    pb = torch.full((n,), float("nan"), dtype=BF16, device=dev)
    ops.adamw(p, m, v, g, pb, lr, b1, b2, eps, wd, step, max_norm=max_norm, norm_sq=nsq, grad_scale=gs)
    R = kcmp.adamw_reference(p0, m0, v0, g, nsq, lr, b1, b2, eps, wd, step, max_norm, gs)
    tag = f"adamw n={n} gradients {gdtype}"
    for name, got in (("m", m), ("v", v), ("p", p), ("p_bf16", pb)):
        kcmp.assert_elementwise(got, *R[name], f"{tag} {name}")
    assert torch.equal(pb, p.to(BF16))
