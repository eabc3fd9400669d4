"""Continuing from a KV cache (ABI 9; DESIGN.md "Continuing from a cache"), the kernels:

  * mg_attn_prefill_cached_bf16 -- a chunk of T new queries per row against the cache, row b's chunk at its own position p_b --
    against an fp32 PyTorch statement of every row, and at p = 0 / T = 1 against the prefill and decode attention;
  * mg_rotary_split_bf16 with pos_stride = 1: the rotated K / V of row b land at p_b + t, every other slot is bit-unchanged."""
import math

import pytest
import torch

import kernel_compare as kcmp

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def rnd(*shape, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def rel(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-12))


def ref_chunk(q, kc, vc, p, T):
    """fp32 statement of one row: q (H, T, 256); query t attends to keys [0, p + t]."""
    k, v = kc[:, : p + T].float().cpu(), vc[:, : p + T].float().cpu()
    sc = q.float().cpu() @ k.transpose(-1, -2) / 16.0
    key = torch.arange(p + T)[None, :]
    sc = sc.masked_fill(key > (p + torch.arange(T))[:, None], float("-inf"))
    return (torch.softmax(sc, -1) @ v).transpose(0, 1).reshape(T, -1)


@pytest.mark.parametrize("T", [1, 5, 32, 33, 130])
def test_chunk_attention_per_row_positions(dev, T):
    from magma_amd import ops
    B, H, Smax = 3, 2, 384
    pos = [0, 37, 190]
    kc = rnd(B, H, Smax, 256, dev=dev, seed=1, scale=0.5).to(BF16)
    vc = rnd(B, H, Smax, 256, dev=dev, seed=2).to(BF16)
    q = rnd(B, H, T, 256, dev=dev, seed=3, scale=0.5).to(BF16)
    d_pos = torch.tensor(pos, dtype=torch.int32, device=dev)
    out = torch.full((B * T, H * 256), float("nan"), dtype=BF16, device=dev)
    ops.attn_prefill_cached(q, kc, vc, out, B, H, T, d_pos, pos_stride=1)
    torch.cuda.synchronize()
    for b, p in enumerate(pos):
        e = rel(out[b * T:(b + 1) * T], ref_chunk(q[b], kc[b], vc[b], p, T))
        assert math.isfinite(e) and e <= 3e-3, f"row {b} (p = {p}, T = {T}): rel-L2 {e:.3e}"
    kcmp.assert_causal_attention(out, q, kc, vc, f"chunk attention T={T}, positions {pos}", p0=d_pos)
    # one shared position (pos_stride 0) reads d_pos[0] for every row
    out0 = torch.empty_like(out)
    ops.attn_prefill_cached(q, kc, vc, out0, B, H, T, d_pos[1:2].contiguous(), pos_stride=0)
    for b in range(B):
        e = rel(out0[b * T:(b + 1) * T], ref_chunk(q[b], kc[b], vc[b], 37, T))
        assert e <= 3e-3, f"shared position, row {b}: rel-L2 {e:.3e}"
    kcmp.assert_causal_attention(out0, q, kc, vc, f"chunk attention T={T}, shared position 37", p0=37)


@pytest.mark.parametrize("inputs", ["self c=1", "self c=2", "tile edges"])
@pytest.mark.parametrize("T", [1, 5, 32, 33, 130])
@pytest.mark.parametrize("Smax,ends", [(384, None), (2048, (1024, 1991, 2048))])
def test_chunk_attention_boundary_inputs(dev, T, inputs, Smax, ends):
    """Keys that make the causal limit of every row count: the key a query appended itself (position p_b + t) dominates its row
    ("self": k = bf16(c q + 0.25 noise)), or only the keys at the edges of the 32-key tiles and the chunk's last key do ("tile
    edges": k = 4 q there).  A limit that is off by one in either direction moves those rows far outside the per-element bound.
    Short contexts (positions 0 / 37 / 190) and long ones whose chunk ENDS at key 1024 (a full tile), 1991 (a partial one) and
    2048 (the end of the cache)."""
    from magma_amd import ops
    B, H = 3, 2
    pos = [0, 37, 190] if ends is None else [e - T for e in ends]
    kc = rnd(B, H, Smax, 256, dev=dev, seed=21, scale=0.5).to(BF16)
    vc = rnd(B, H, Smax, 256, dev=dev, seed=22).to(BF16)
    q = rnd(B, H, T, 256, dev=dev, seed=23, scale=0.5).to(BF16)
    noise = rnd(B, H, T, 256, dev=dev, seed=24, scale=0.25)
    for b, p in enumerate(pos):
        if inputs == "tile edges":
            ts = [t for t in range(T) if (p + t) % 32 in (0, 31) or t == T - 1]
            kc[b, :, [p + t for t in ts]] = (q[b, :, ts].float() * 4).to(BF16)
        else:
            kc[b, :, p:p + T] = (float(inputs[-1]) * q[b].float() + noise[b]).to(BF16)
    d_pos = torch.tensor(pos, dtype=torch.int32, device=dev)
    out = torch.full((B * T, H * 256), float("nan"), dtype=BF16, device=dev)
    ops.attn_prefill_cached(q, kc, vc, out, B, H, T, d_pos, pos_stride=1)
    kcmp.assert_causal_attention(out, q, kc, vc, f"chunk attention T={T}, positions {pos}, {inputs}", p0=d_pos)
    for b, p in enumerate(pos):
        assert rel(out[b * T:(b + 1) * T], ref_chunk(q[b], kc[b], vc[b], p, T)) <= 3e-3


def test_chunk_attention_strided_queries_and_wide_output(dev):
    """q as a strided view ([B, T, H, 256] storage) and out as a column range of a wider row."""
    from magma_amd import ops
    B, H, Smax, T = 2, 2, 256, 20
    pos = [64, 3]
    kc = rnd(B, H, Smax, 256, dev=dev, seed=4, scale=0.5).to(BF16)
    vc = rnd(B, H, Smax, 256, dev=dev, seed=5).to(BF16)
    qs = rnd(B, T, H, 256, dev=dev, seed=6, scale=0.5).to(BF16)
    q = qs.permute(0, 2, 1, 3)
    wide = torch.zeros(B * T, H * 256 + 64, dtype=BF16, device=dev)
    ops.attn_prefill_cached(q, kc, vc, wide[:, : H * 256], B, H, T, torch.tensor(pos, dtype=torch.int32, device=dev), pos_stride=1)
    for b, p in enumerate(pos):
        assert rel(wide[b * T:(b + 1) * T, : H * 256], ref_chunk(q[b], kc[b], vc[b], p, T)) <= 3e-3
    kcmp.assert_causal_attention(wide[:, : H * 256], q, kc, vc, "chunk attention, strided q, wide output", p0=torch.tensor(pos))
    assert torch.equal(wide[:, H * 256:], torch.zeros_like(wide[:, H * 256:]))


def test_chunk_attention_agrees_with_prefill_and_decode(dev):
    from magma_amd import ops
    B, H, Smax = 2, 2, 256
    # p = 0: the whole causal prefill of T rows, as attn_fwd_rows computes it -- to the bit: the two kernels are one text, and at
    # p = 0 they do the same arithmetic in the same order.  T = 128 is a full query block, 130 the first rows of the next one
    kc = rnd(B, H, Smax, 256, dev=dev, seed=7, scale=0.5).to(BF16)
    vc = rnd(B, H, Smax, 256, dev=dev, seed=8).to(BF16)
    for T in (130, 128, 77):
        q = rnd(B, H, T, 256, dev=dev, seed=9, scale=0.5).to(BF16)
        out = torch.empty(B * T, H * 256, dtype=BF16, device=dev)
        ops.attn_prefill_cached(q, kc, vc, out, B, H, T, torch.zeros(B, dtype=torch.int32, device=dev), pos_stride=1)
        k, v = kc[:, :, :T].contiguous(), vc[:, :, :T].contiguous()
        ref = torch.empty_like(out)
        ops.attn_fwd_rows(ops.AttnRows.of_bhsd(q.contiguous(), k, v), ref)
        assert rel(out, ref) <= 3e-3, f"T = {T}"
        assert torch.equal(out, ref), f"T = {T}: {int((out != ref).sum())} elements differ from attn_fwd_rows"
        kcmp.assert_causal_attention(out, q, k, v, f"chunk attention at p = 0, T = {T}")
        kcmp.assert_causal_attention(ref, q, k, v, f"attn_fwd_rows on the same operands, T = {T}")
    # T = 1 (q: the first query of the T = 77 chunk): one query per row at its own position, as attn_decode computes it
    pos = [5, 200]
    d_pos = torch.tensor(pos, dtype=torch.int32, device=dev)
    q1 = q[:, :, :1].contiguous()
    o1 = torch.empty(B, H * 256, dtype=BF16, device=dev)
    ops.attn_prefill_cached(q1, kc, vc, o1, B, H, 1, d_pos, pos_stride=1)
    r1 = torch.empty_like(o1)
    ops.attn_decode(q1, kc, vc, r1, B, H, d_pos, pos_stride=1)
    for b in range(B):
        assert rel(o1[b], r1[b]) <= 3e-3, f"row {b}"
    kcmp.assert_causal_attention(o1, q1, kc, vc, "chunk attention, T = 1", p0=d_pos)
    kcmp.assert_causal_attention(r1, q1, kc, vc, "attn_decode on the same operands", p0=d_pos, p_dtype=torch.float32, n_rescale=0)


def test_chunk_attention_argument_checks(dev):
    from magma_amd import ops
    B, H, Smax, T = 2, 2, 64, 4
    kc = torch.zeros(B, H, Smax, 256, dtype=BF16, device=dev)
    q = torch.zeros(B, H, T, 256, dtype=BF16, device=dev)
    out = torch.empty(B * T, H * 256, dtype=BF16, device=dev)
    d_pos = torch.zeros(B, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ops.attn_prefill_cached(q, kc, kc, out[:-1], B, H, T, d_pos, pos_stride=1)
    with pytest.raises(ValueError):
        ops.attn_prefill_cached(q.float(), kc, kc, out, B, H, T, d_pos, pos_stride=1)
    with pytest.raises(ValueError):
        ops.attn_prefill_cached(q, kc[:, :, :2], kc[:, :, :2], out, B, H, T, d_pos, pos_stride=1)
    with pytest.raises(ValueError):
        ops.attn_prefill_cached(q, kc, kc, out, B, H, T, d_pos[:1], pos_stride=1)


def test_rotary_append_per_row_positions(dev):
    from magma_amd import ops
    from oracle.model import apply_rotary, rotary_tables
    B, H, Smax, rot, T = 3, 2, 256, 64, 6
    pos = [0, 37, 190]
    d = H * 256
    kc0 = rnd(B, H, Smax, 256, dev=dev, seed=11, scale=0.5).to(BF16)
    vc0 = rnd(B, H, Smax, 256, dev=dev, seed=12).to(BF16)
    qkv = rnd(B * T, 3 * d, dev=dev, seed=13, scale=0.5).to(BF16)
    sin_t, cos_t = rotary_tables(rot, Smax)
    sin_t, cos_t = sin_t.to(dev).contiguous(), cos_t.to(dev).contiguous()
    kc, vc = kc0.clone(), vc0.clone()
    q = torch.empty(B, H, T, 256, dtype=BF16, device=dev)
    ops.rotary_split(qkv, B, T, H, rot, sin_t, cos_t, q, kc, vc, d_pos=torch.tensor(pos, dtype=torch.int32, device=dev), pos_stride=1)
    x = qkv.view(B, T, 3, H, 256).float().cpu()
    for b, p in enumerate(pos):
        pt = torch.arange(p, p + T)
        k_new = apply_rotary(x[b:b + 1, :, 1], pt, rot)[0].transpose(0, 1)          # (H, T, 256)
        q_new = apply_rotary(x[b:b + 1, :, 0], pt, rot)[0].transpose(0, 1)
        assert rel(kc[b, :, p:p + T], k_new) <= 3e-3 and rel(q[b], q_new) <= 3e-3, f"row {b}"
        assert torch.equal(vc[b, :, p:p + T].float().cpu(), x[b, :, 2].transpose(0, 1)), f"appended v, row {b}"
        keep = torch.ones(Smax, dtype=torch.bool)
        keep[p:p + T] = False
        assert torch.equal(kc[b][:, keep], kc0[b][:, keep]) and torch.equal(vc[b][:, keep], vc0[b][:, keep]), f"row {b}: other slots"
    # a chunk running past Smax writes nothing there (and nothing elsewhere)
    kc2, vc2 = kc0.clone(), vc0.clone()
    ops.rotary_split(qkv, B, T, H, rot, sin_t, cos_t, q, kc2, vc2, d_pos=torch.tensor([Smax - 2] * B, dtype=torch.int32, device=dev),
                     pos_stride=1)
    assert torch.equal(kc2[:, :, : Smax - 2], kc0[:, :, : Smax - 2]) and torch.equal(vc2[:, :, : Smax - 2], vc0[:, :, : Smax - 2])
