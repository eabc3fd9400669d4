"""The attention backward of the trainable CLIP ViT encoder, mg_attn_small_bwd_bf16 (attn_small_bwd_kernel in csrc/elementwise.hip),
per element: dq, dk and dv each against kernel_compare.attn_small_backward_reference, whose bound is derived from the kernel's
own steps (tests/test_kernel_compare_cpu.py keeps what that bound accepts and what it refuses).  The whole-tensor norm of
tests/test_variants_gpu.py::test_attn_small_backward stays beside it; it accepts a dq or dk that is 2 % too large.

Shapes and input families are kernel_compare.ATTN_SMALL_BWD_SHAPES / ATTN_SMALL_BWD_FAMILIES; inputs are built on the CPU from
fixed seeds and each reference is formed once."""
import functools

import pytest
import torch

import kernel_compare as kcmp

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
GRADS = ("dq", "dk", "dv")


@functools.lru_cache(maxsize=None)
def case(family, B, S, H):
    """(qkv, d_out, reference) on the CPU; shared, read-only."""
    qkv, d_out = kcmp.attn_small_backward_inputs(family, B, S, H)
    return qkv, d_out, kcmp.attn_small_backward_reference(qkv, d_out, B, S, H)


def run_bwd(dev, qkv, d_out, B, S, H):
    """The kernel's d_qkv [B*S, 3*H*64] and its (dq, dk, dv) as [B, H, S, 64] views, on the CPU."""
    from magma_amd import ops
    got = ops.attn_small_bwd(qkv.to(dev), d_out.to(dev), B, S, H).cpu()
    return got, dict(zip(GRADS, kcmp.heads_of(got, B, S, H)))


@pytest.mark.parametrize("family", kcmp.ATTN_SMALL_BWD_FAMILIES)
@pytest.mark.parametrize("B,S,H", kcmp.ATTN_SMALL_BWD_SHAPES)
def test_attn_small_backward_elementwise(dev, B, S, H, family):
    """dq, dk and dv separately, per element; a second launch on the same inputs gives the same bits (no atomics);
    one token: dq = dk = 0 and dv = dO exactly; class rows only: dq is exactly zero outside row 0."""
    qkv, d_out, R = case(family, B, S, H)
    rows, got = run_bwd(dev, qkv, d_out, B, S, H)
    for name in GRADS:
        kcmp.assert_elementwise(got[name], *R[name], f"attn_small_bwd {name} B={B} S={S} H={H}, {family}")
    again, _ = run_bwd(dev, qkv, d_out, B, S, H)
    assert torch.equal(rows, again), "two launches on the same inputs differ"
    if S == 1:
        assert not got["dq"].any() and not got["dk"].any(), "one token: softmax is 1, dS is 0"
        assert torch.equal(got["dv"], kcmp.heads_of(d_out, B, S, H)[0]), "one token: dv = dO"
    if family == "class rows only":
        assert not got["dq"][:, :, 1:].any(), "dO is zero outside row 0: so are dP, dS and dq there"


@pytest.mark.parametrize("h", [0, 5, 11])
def test_attn_small_backward_head_addressing(dev, h):
    """dO of one head zeroed: that head's columns of dq, dk and dv are exactly zero, every other head keeps its bits."""
    B, S, H = 2, 50, 12
    qkv, d_out, _ = case("i.i.d.", B, S, H)
    _, full = run_bwd(dev, qkv, d_out, B, S, H)
    d_cut = d_out.clone()
    d_cut.view(B * S, H, 64)[:, h] = 0
    _, cut = run_bwd(dev, qkv, d_cut, B, S, H)
    others = [i for i in range(H) if i != h]
    for name in GRADS:
        assert full[name][:, h].any(), "the case must have something to lose"
        assert not cut[name][:, h].any(), f"{name} of head {h} is not zero although its dO is"
        assert torch.equal(cut[name][:, others], full[name][:, others]), f"{name}: zeroing head {h} changed another head"


@pytest.mark.parametrize("op,S,limit", [("attn_small_bwd", 65, 64), ("attn_small_bwd", 0, 64), ("attn_small", 257, 256), ("attn_small", 0, 256)])
def test_attn_small_refuses_sequences_outside_its_lds(dev, op, S, limit):
    """The backward keeps the whole head in LDS up to S = 64, the forward up to 256: one more, or no token at all, is refused
    with the library's error, which names the limit, before anything is launched."""
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    qkv = torch.zeros(S, 3 * 64, dtype=BF16, device=dev)
    with pytest.raises(MagmaHipError, match=rf"need 0 < S <= {limit} \(head dim 64\)"):
        if op == "attn_small":
            ops.attn_small(qkv, 1, S, 1)
        else:
            ops.attn_small_bwd(qkv, torch.zeros(S, 64, dtype=BF16, device=dev), 1, S, 1)
    torch.cuda.synchronize()
