"""mg_attn_prefill_fp8 (csrc/attention_fwd32_fp8.hip) per element, on inputs where each part of its causal limit decides the output.

The kernel's limit has six parts -- lim0 = min(qrow, S - 1) - 4 hi against the permuted key order, 64-key tiles, 128-query blocks,
n_act per wave, the clamped tile index of a block with fewer tiles than the prologue issues, the deferred-maximum rescale -- and
i.i.d. inputs see none of them: a long softmax row averages ~S values (tests/test_kernel_compare_cpu.py keeps the figures of the
seeded faults and names the input kind that catches each).  Reference: fp64 causal attention on the DEQUANTISED operands, bound:
kernel_compare.fp8_attention_bound, derived from the measured arithmetic of v_mfma_scale_f32_32x32x64_f8f6f4."""
import math

import pytest
import torch

import kernel_compare as kcmp

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
ROT = 64


def _tables(S, dev):
    inv = 1.0 / (10000 ** (torch.arange(0, ROT, 2, dtype=torch.float32, device=dev) / ROT))
    ang = torch.arange(S + 3, dtype=torch.float32, device=dev)[:, None] * inv[None, :]
    return ang.sin().contiguous(), ang.cos().contiguous()


def _run(ops, q, k, v, dev):
    """q, k, v bf16 [B, H, S, 256] before the rotary -> (op, out [B*S, H*256] bf16, lse [B, H, S]) through mg_rotary_split_fp8
    (rot_dim 64) and mg_attn_prefill_fp8.  The output starts as NaN: a row the kernel does not write fails the comparison."""
    B, H, S, _ = q.shape
    sin_t, cos_t = _tables(S, dev)
    op = ops.rotary_split_fp8(kcmp.qkv_rows(q, k, v).to(dev), B, S, H, ROT, sin_t, cos_t)
    out = torch.full((B * S, H * 256), float("nan"), dtype=BF16, device=dev)
    lse = torch.full((B, H, S), float("nan"), dtype=torch.float32, device=dev)
    ops.attn_prefill_fp8(op, out, lse=lse)
    return op, out, lse


# S: fewer tiles than the three the prologue issues (1 .. 128); a partial last 64-key tile (all but 64, 128, 1024, 2048); a partial
# last 128-query block (all but 128, 1024, 2048); waves with n_act < ntiles (every block of 65 rows or more); B * H >= 3 at 129, 300
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 127, 128, 129, 191, 193, 300, 385, 1024, 2048])
@pytest.mark.parametrize("kind", kcmp.FP8_ATTN_INPUTS)
def test_fp8_attention_boundary_inputs(dev, kind, S):
    """Output and lse per element for the input kinds of kernel_compare.fp8_attention_inputs (different data per batch row and
    head).  "next key" puts k[i + 1] = 2 q[i] into the dimensions the rotary leaves alone (>= 64), so the kernel is called as
    in the model, with rot_dim = 64, for every kind."""
    from magma_amd import ops
    B = 2 if S in (129, 300) else 1
    q, k, v = kcmp.fp8_attention_inputs(kind, (B, 2, S, 256), seed=91 + S, device=dev, rot_dim=ROT)
    op, out, lse = _run(ops, q, k, v, dev)
    kcmp.assert_causal_attention_fp8(out, op, f"attn_prefill_fp8 {kind} B={B} H=2 S={S}", lse=lse)


@pytest.mark.parametrize("S", [300, 1024])
@pytest.mark.parametrize("gain,crosses", [(2.0, True), (0.85, False)])
def test_fp8_attention_deferred_maximum(dev, gain, crosses, S):
    """A late key that dominates the last 40 queries: k[S - 40] = gain * u and q[r] += u for r >= S - 40, u of scale 0.5 in the
    dimensions >= 64 (|u|^2 ~ 48: a score of 3 gain nats = 4.3 gain in log2 units above i.i.d. scores of spread ~1).  gain 2:
    the tile of that key lies 5.9 .. 9.4 above the kept maximum of those rows (more than P_DEFER = 4): the maximum moves and
    everything accumulated before is rescaled; gain 0.85: 1.4 .. 3.4 above, the maximum stays and the tile's probabilities
    exceed 1 (the e4m3 operand holds up to 16).  Which of the two happens is checked on the exact scores; then output and lse per element."""
    from magma_amd import ops
    g = torch.Generator().manual_seed(7)
    shape = (1, 2, S, 256)
    q = torch.randn(*shape, generator=g) * 0.5
    k = torch.randn(*shape, generator=g) * 0.5
    v = torch.randn(*shape, generator=g)
    u = torch.randn(1, 2, 1, 256 - ROT, generator=g) * 0.5
    j = S - 40
    q[:, :, j:, ROT:] += u
    k[:, :, j, ROT:] = gain * u[:, :, 0]
    op, out, lse = _run(ops, q.to(BF16), k.to(BF16), v.to(BF16), dev)
    qd, kd, _ = op.dequant()
    vis = kcmp.causal_mask(S, S, 0, dev)
    for h in range(2):
        t2 = kcmp.f64(qd[0, h]) @ kcmp.f64(kd[0, h]).t() * (math.log2(math.e) / 16.0)
        moved, over = kcmp.deferred_maximum_trace(t2, vis)
        tile = j // kcmp.FP8_ATTN_TILE
        if crosses:
            assert bool(moved[j:, tile].all()), "the late key was meant to move the deferred maximum of every row that sees it"
        else:
            assert not bool(moved[j:, tile:].any()) and bool(over[j:, tile].all()), "the late key was meant to stay under the threshold"
    kcmp.assert_causal_attention_fp8(out, op, f"attn_prefill_fp8 late key gain {gain} S={S}", lse=lse)


@pytest.mark.parametrize("S", [57, 385])
def test_fp8_attention_producer_padding(dev, S):
    """What the attention kernel multiplies by P = 0 must still be finite: mg_rotary_split_fp8 writes zero bytes for the keys >= S of
    the last V^T tile, the unit scale (127) for V^T blocks that are all padding, and eq / ek beyond S are the unit scale."""
    from magma_amd import ops
    B, H = 2, 2
    q, k, v = kcmp.fp8_attention_inputs("self c=1", (B, H, S, 256), seed=5, device=dev)
    sin_t, cos_t = _tables(S, dev)
    op = ops.rotary_split_fp8(kcmp.qkv_rows(q, k, v).to(dev), B, S, H, ROT, sin_t, cos_t)
    order = torch.tensor(kcmp.fp8_attn_key_order(), device=dev)          # key (within the tile) of byte position 32 hi + 16 b + r ...
    byte_of_key = torch.empty(64, dtype=torch.long, device=dev)
    pos = torch.tensor([32 * hi + 16 * b + r for b in range(2) for hi in range(2) for r in range(16)], device=dev)
    byte_of_key[order] = pos                                             # ... inverted: the byte that holds a key
    nt = (S + 63) // 64
    pad_keys = torch.arange(S, nt * 64, device=dev) - (nt - 1) * 64
    assert pad_keys.numel() > 0
    assert int(op.v8t[:, :, nt - 1][..., byte_of_key[pad_keys]].abs().max()) == 0, "V^T bytes of the keys >= S"
    assert int((op.v8t[:, :, nt - 1][..., byte_of_key[torch.arange(0, S - (nt - 1) * 64, device=dev)]] != 0).sum()) > 0
    sv = op.sv8.view(B, H, nt, 2, 32, 8)                                 # [key block][d % 32][d / 32]
    for b in range(2):
        if (nt - 1) * 64 + 32 * b >= S:
            assert bool((sv[:, :, nt - 1, b] == 127).all()), "scale of an all-padding V^T block"
    assert bool((op.eq[:, :, S:] == 127).all()) and bool((op.ek[:, :, S:] == 127).all())
    assert bool((op.sv8 < 255).all()) and bool((op.eq < 255).all()) and bool((op.ek < 255).all())        # 255 is E8M0's NaN


def test_fp8_attention_wide_and_mx_output_on_a_boundary_input(dev):
    """The wide-row and MX-copy forms of the call write the same bf16 bits as the plain one, on an input where the last block is
    partial and its rows depend on their newest key (S = 193, "tile edges")."""
    from magma_amd import ops
    B, H, S = 1, 2, 193
    d = H * 256
    q, k, v = kcmp.fp8_attention_inputs("tile edges", (B, H, S, 256), seed=17, device=dev)
    op, out, _ = _run(ops, q, k, v, dev)
    kcmp.assert_causal_attention_fp8(out, op, "attn_prefill_fp8 tile edges S=193 (plain call)")
    wide = torch.full((B * S, d + 136), float("nan"), dtype=BF16, device=dev)
    ops.attn_prefill_fp8(op, wide[:, :d])
    assert torch.equal(wide[:, :d], out) and bool(torch.isnan(wide[:, d:]).all())
    mx = ops.mx_empty(B * S, d, dev)
    out_b = torch.empty_like(out)
    ops.attn_prefill_fp8(op, out_b, mx_out=mx)
    qref, sref = ops.quantize_mx_fp8(out)
    assert torch.equal(out_b, out) and torch.equal(mx[0], qref) and torch.equal(mx[1], sref)
