"""Full-size (BASELINE.json shapes) checks through size-independent properties -- the CPU oracle cannot
run d = 4096 / S = 2048 in seconds, so at these sizes parity is argued from invariants of the maths:

* KV-cache consistency: prefill(S0 tokens) + one decode step == prefill(S0 + 1 tokens) at the new position.
  The two sides share no GEMM / attention kernel (tile GEMM + split-K + flash attention vs the
  weight-streaming GEMV with folded LayerNorm + decode attention), so agreement pins both.
* batch invariance: identical rows in -> bit-identical rows out.
* flash attention at S = 2048: causality is bit-exact (keys after a query cannot change it), V = 1 gives 1,
  the saved log-sum-exp matches a direct fp32 evaluation, and the backward satisfies the scaling identity
  sum(q . dq) == sum(k . dk) per head (d/dalpha of the loss under q -> alpha q equals that under k -> alpha k).
* tile GEMMs at training shapes against torch fp32 on the same device, including the split-K path."""
import pytest
import torch

import kernel_compare as kcmp

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.fixture(scope="module")
def wide_model(dev):
    """MAGMA_v1 at full width (d = 4096, 16 heads, ff = 16384, V = 50258, RN50x16 trunk), 2 GPT-J blocks."""
    from magma_amd import Magma
    from magma_amd.language_model import GPTJConfig
    torch.manual_seed(7)
    model = Magma("MAGMA_v1", device=dev, lm_config=GPTJConfig(num_layers=2, vocab_size=50258))
    model.eval()
    return model


def test_kv_cache_consistency_full_width(wide_model, dev):
    model = wide_model
    g = torch.Generator(device=dev).manual_seed(3)
    B = 8
    images = torch.randn(B, 3, 224, 224, device=dev, generator=g).to(BF16)
    prompt = torch.randint(0, 50256, (B, 9), device=dev, generator=g)
    with torch.no_grad():
        emb = model.embed([images, prompt])                                   # (8, 49 + 9, 4096)
        assert emb.shape == (B, 58, 4096)
        full = model.lm(inputs_embeds=emb, use_cache=True).logits[:, -1].float()
        pre = model.lm(inputs_embeds=emb[:, :-1].contiguous(), use_cache=True, cache_hint=8)
        step = model.lm(input_ids=prompt[:, -1:], use_cache=True, past_key_values=pre.past_key_values)
        inc = step.logits[:, -1].float()
    assert torch.isfinite(full).all() and torch.isfinite(inc).all()
    # two independent bf16 kernel stacks: agreement to bf16 rounding of the activations
    assert rel(inc, full) < 2e-2, rel(inc, full)
    top2 = full.topk(2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 0.05 * full.std(dim=-1)
    assert bool((inc.argmax(-1)[clear] == full.argmax(-1)[clear]).all())


def test_batch_rows_are_independent_full_width(wide_model, dev):
    model = wide_model
    g = torch.Generator(device=dev).manual_seed(4)
    img = torch.randn(1, 3, 224, 224, device=dev, generator=g).to(BF16)
    ids = torch.randint(0, 50256, (1, 8), device=dev, generator=g)
    with torch.no_grad():
        out8 = model.lm(inputs_embeds=model.embed([img.expand(8, -1, -1, -1).contiguous(), ids.expand(8, -1).contiguous()]),
                        use_cache=True).logits[:, -1].float()
        out1 = model.lm(inputs_embeds=model.embed([img, ids]), use_cache=True).logits[:, -1].float()
    for r in range(1, 8):
        assert torch.equal(out8[r], out8[0]), f"row {r} differs from row 0"
    assert rel(out8[0], out1[0]) < 1e-2          # other tile / split-K configuration: rounding-level difference only


def test_flash_attention_properties_s2048(dev):
    from magma_amd import ops
    B, H, S = 1, 2, 2048
    d = H * 256
    g = torch.Generator(device=dev).manual_seed(9)
    q = (torch.randn(B, H, S, 256, device=dev, generator=g) * 0.5).to(BF16)
    k = (torch.randn(B, H, S, 256, device=dev, generator=g) * 0.5).to(BF16)
    v = torch.randn(B, H, S, 256, device=dev, generator=g).to(BF16)
    hs = H * S * 256

    def fwd(q, k, v):
        vt = ops.head_transpose(v, B, H, S, sb=hs, ss=256, sh=S * 256)
        out = torch.empty(B * S, d, dtype=BF16, device=dev)
        lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
        ops.attn_prefill(q, k, vt, out, B, H, S, lse=lse)
        return out, lse

    out, lse = fwd(q, k, v)
    # causality, bit-exact: whatever sits at keys >= 1024 cannot reach queries < 1024
    k2, v2 = k.clone(), v.clone()
    k2[:, :, 1024:] = (torch.randn(B, H, S - 1024, 256, device=dev, generator=g) * 3).to(BF16)
    v2[:, :, 1024:] = 1000.0
    out2, lse2 = fwd(q, k2, v2)
    assert torch.equal(out2.view(B, S, d)[:, :1024], out.view(B, S, d)[:, :1024])
    assert torch.equal(lse2[:, :, :1024], lse[:, :, :1024])
    # softmax rows sum to one
    ones, _ = fwd(q, k, torch.ones_like(v))
    assert float((ones.float() - 1).abs().max()) < 1e-2
    # saved log-sum-exp against a direct fp32 evaluation on a few query rows
    for qi in (0, 1, 31, 32, 1000, 2047):
        s = (q[0, 1, qi].float() @ k[0, 1, : qi + 1].float().t()) / 16.0
        assert abs(float(torch.logsumexp(s, 0)) - float(lse[0, 1, qi])) < 2e-3, qi
    # full output against torch fp32 on the device
    sc = (q.float() @ k.float().transpose(-1, -2)) / 16.0
    sc = sc.masked_fill(~torch.ones(S, S, dtype=torch.bool, device=dev).tril(), float("-inf"))
    ref = (torch.softmax(sc, -1) @ v.float()).permute(0, 2, 1, 3).reshape(B * S, d)
    assert rel(out, ref) < 1e-2, rel(out, ref)
    kcmp.assert_causal_attention(out, q, k, v, "flash attention S=2048, i.i.d.", lse=lse)
    # with i.i.d. inputs a last row without its own key is invisible (a row of 2048 keys averages): each query's own key dominates
    for c in (1.0, 2.0):
        qs, ks, vs = kcmp.self_dominant_qkv((B, H, S, 256), c, seed=19, device=dev)
        outs, lses = fwd(qs, ks, vs)
        kcmp.assert_causal_attention(outs, qs, ks, vs, f"flash attention S=2048, self-dominant c={c}", lse=lses)
    ke = kcmp.dominant_edge_keys(q, k)
    oute, lsee = fwd(q, ke, v)
    kcmp.assert_causal_attention(oute, q, ke, v, "flash attention S=2048, dominant tile-edge keys", lse=lsee)
    # backward: scaling identity per head, and dv against autograd
    dO = torch.randn(B * S, d, device=dev, generator=g).to(BF16)
    qt = ops.head_transpose(q, B, H, S, sb=hs, ss=256, sh=S * 256)
    kt = ops.head_transpose(k, B, H, S, sb=hs, ss=256, sh=S * 256)
    dOt = ops.head_transpose(dO, B, H, S, sb=S * d, ss=d, sh=256)
    dq, dk, dv = ops.attn_bwd(q, k, v, qt, kt, dO, dOt, out, lse, B, H, S)
    lhs = (q.float() * dq.float()).sum(dim=(2, 3))
    rhs = (k.float() * dk.float()).sum(dim=(2, 3))
    scale = (q.float() * dq.float()).abs().sum(dim=(2, 3))
    assert float(((lhs - rhs).abs() / scale).max()) < 5e-3, (lhs, rhs)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    sc = (qf @ kf.transpose(-1, -2)) / 16.0
    sc = sc.masked_fill(~torch.ones(S, S, dtype=torch.bool, device=dev).tril(), float("-inf"))
    (torch.softmax(sc, -1) @ vf).permute(0, 2, 1, 3).reshape(B * S, d).backward(dO.float())
    assert rel(dq, qf.grad) < 1.5e-2 and rel(dk, kf.grad) < 1.5e-2 and rel(dv, vf.grad) < 1.5e-2
    kcmp.assert_attention_backward(dq, dk, dv, q, k, v, dO, out, lse, "attn_bwd S=2048")


@pytest.mark.parametrize("M,N,K,why", [(4096, 4096, 16384, "fc_out slice, 256x256 kernel"),
                                       (456, 4096, 16384, "prefill fc_out, split-K"),
                                       (456, 1024, 4096, "prefill adapter-down, 16-way split-K"),
                                       (8192, 1024, 4096, "adapter-down, training rows")])
def test_tile_gemm_training_shapes(dev, M, N, K, why):
    from magma_amd import ops
    g = torch.Generator(device=dev).manual_seed(M + N)
    a = torch.randn(M, K, device=dev, generator=g).to(BF16)
    w = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(BF16)
    bias = torch.randn(N, device=dev, generator=g)
    res = torch.randn(M, N, device=dev, generator=g).to(BF16)
    lin = ops.PackedLinear(w, bias=bias)
    ref = a.float() @ w.float().t() + bias + res.float()
    out = ops.gemm(a, lin, residuals=(res,))
    assert rel(out, ref) < 4e-3, (why, rel(out, ref))
    kcmp.assert_linear(out, f"tile GEMM {M}x{N}x{K} ({why})", a, w, bias=bias, residuals=(res,))
    again = ops.gemm(a, lin, residuals=(res,))
    assert torch.equal(out, again), f"{why}: not deterministic"
