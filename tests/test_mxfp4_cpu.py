"""OCP MXFP4 weight quantiser and pack of the W4A16 decode GEMV (ops.quantize_mx_fp4 / PackedLinearW4), on the CPU: the
rounding grid and the shared-exponent rule on hand-built blocks, exact dequantisation, the tiling round trip, and the weight
error of the rule on Gaussian weights."""
import pytest
import torch

from magma_amd import ops

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def codes_of(packed):
    """[N, K/2] bytes -> [N, K] nibbles, element 2i from the low nibble of byte i."""
    return torch.stack([packed & 15, packed >> 4], dim=-1).reshape(packed.shape[0], -1)


def block(values, fill=0.0):
    """One row of one 32-element block holding ``values`` first."""
    row = torch.full((1, 32), fill, dtype=torch.float32)
    row[0, : len(values)] = torch.tensor(values, dtype=torch.float32)
    return row


@pytest.mark.parametrize("e", [-20, -3, 0, 5, 60])
def test_scale_rule_and_grid(e):
    s = 2.0 ** e
    # amax exactly 6 * 2^e: the shared exponent is e, every grid value is kept, with its sign
    vals = [6.0, -6.0, 4.0, -3.0, 2.0, 1.5, -1.0, 0.5, 0.0]
    c, sc = ops.quantize_mx_fp4(block([v * s for v in vals]))
    assert sc.shape == (1, 1) and int(sc[0, 0]) == e + 127
    want = [GRID.index(abs(v)) | (8 if v < 0 else 0) for v in vals]
    assert codes_of(c)[0, : len(vals)].tolist() == want and not codes_of(c)[0, len(vals):].any()
    # amax just above 7 * 2^e: floor(log2) is still e + 2, the element saturates at 6 (never 8, never a larger scale)
    c, sc = ops.quantize_mx_fp4(block([7.001 * s, -7.5 * s, 5.1 * s]))
    assert int(sc[0, 0]) == e + 127 and codes_of(c)[0, :3].tolist() == [7, 15, 7]
    # amax just below 4 * 2^e belongs to the exponent below: 3.99 / 0.5 = 7.98 -> saturates at 6 * 2^(e-1)
    c, sc = ops.quantize_mx_fp4(block([3.99 * s]))
    assert int(sc[0, 0]) == e - 1 + 127 and int(codes_of(c)[0, 0]) == 7


def test_ties_go_to_the_even_code():
    # (amax 6 pins the exponent to 0)  0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4: codes 0 2 2 4 4 6 6
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    c, sc = ops.quantize_mx_fp4(block([6.0] + ties + [-t for t in ties]))
    assert int(sc[0, 0]) == 127
    got = codes_of(c)[0, 1:15].tolist()
    assert got[:7] == [0, 2, 2, 4, 4, 6, 6]
    assert got[7:] == [0, 10, 10, 12, 12, 14, 14]          # a value that rounds to zero is +0
    # just off the ties, both sides
    eps = 1e-3
    c, _ = ops.quantize_mx_fp4(block([6.0] + [t - eps for t in ties] + [t + eps for t in ties]))
    got = codes_of(c)[0, 1:15].tolist()
    assert got[:7] == [0, 1, 2, 3, 4, 5, 6] and got[7:] == [1, 2, 3, 4, 5, 6, 7]


def test_zero_block_and_exponent_clamp():
    w = torch.cat([block([]), block([6.0]), block([2.0 ** -140, -(2.0 ** -126)]), block([3.0e38, -2.0e38, 2.0 ** 126])], dim=1)
    c, sc = ops.quantize_mx_fp4(w)
    cd = codes_of(c)
    assert not cd[0, :32].any() and int(sc[0, 0]) == 127                     # zero block: zero codes
    # tiny: floor(log2 amax) - 2 = -128 is clamped to -125; 2^-126 / 2^-125 = 0.5 (code 1), 2^-140 rounds to +0
    assert int(sc[0, 2]) == 2 and cd[0, 64:66].tolist() == [0, 9]
    # huge: 3e38 ~ 1.76 * 2^127 -> e = 125 is clamped to 124, the elements saturate; 2^126 = 4 * 2^124 (code 6)
    assert int(sc[0, 3]) == 251 and cd[0, 96:99].tolist() == [7, 15, 6]
    d = ops.dequantize_mx_fp4(c, sc)
    assert torch.isfinite(d).all()
    nz = d[d != 0].abs()
    assert float(nz.min()) >= 2.0 ** -126, "a non-zero dequantised value must be a normal bf16"
    assert torch.equal(d.to(torch.bfloat16).float(), d)
    assert d[0, 65] == -(2.0 ** -126) and d[0, 96] == 6 * 2.0 ** 124


def test_element_2i_is_the_low_nibble():
    c, _ = ops.quantize_mx_fp4(block([6.0, 0.5, 1.0, -1.5]))
    assert c[0, :2].tolist() == [7 | (1 << 4), 2 | (11 << 4)]


@pytest.fixture(scope="module")
def gaussian():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(1024, 4096, generator=g) * 0.05
    return w, ops.quantize_mx_fp4(w)


def test_dequantisation_is_exact_and_idempotent(gaussian):
    w, (c, sc) = gaussian
    d = ops.dequantize_mx_fp4(c, sc)
    assert torch.equal(d.to(torch.bfloat16).float(), d), "every e2m1 value times a power of two is a bf16 value"
    c2, sc2 = ops.quantize_mx_fp4(d)
    assert torch.equal(c2, c) and torch.equal(sc2, sc)
    # bf16 input: the quantiser reads the same values whatever dtype carries them
    cb, sb = ops.quantize_mx_fp4(d.to(torch.bfloat16))
    assert torch.equal(cb, c) and torch.equal(sb, sc)


def test_gaussian_weight_error(gaussian):
    """Relative L2 weight error of the OCP rule on N(0, 0.05^2) weights (1024, 4096): 0.118 measured with a restatement of the
    rule; a quantiser that wastes a bit or picks the wrong exponent falls outside [0.10, 0.13]."""
    w, (c, sc) = gaussian
    err = float((ops.dequantize_mx_fp4(c, sc) - w).norm() / w.norm())
    print("MXFP4 relative L2 weight error", err)
    assert 0.10 <= err <= 0.13, err


@pytest.mark.parametrize("N,K", [(1000, 1024), (7, 512), (48, 2048)])
def test_tiling_round_trip(N, K):
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g) * 0.05
    c, sc = ops.quantize_mx_fp4(w)
    lin = ops.PackedLinearW4(w, bias=torch.ones(N))
    n16 = (N + 15) // 16
    assert (lin.N, lin.K, lin.Kp) == (N, K, K) and lin.bias.dtype == torch.float32
    assert lin.ft.dtype == torch.uint8 and lin.ft.numel() == n16 * 16 * K // 2 and lin.ft.is_contiguous()
    assert lin.scales.dtype == torch.uint8 and lin.scales.numel() == n16 * 16 * K // 32 and lin.scales.is_contiguous()
    c2, sc2 = ops.untile_mx_fp4(lin.ft, lin.scales, N)
    assert torch.equal(c2, c) and torch.equal(sc2, sc)
    assert torch.equal(lin.dequant(), ops.dequantize_mx_fp4(c, sc))
    # the documented layout, read straight from the flat bytes: lane = kq*16 + n, bytes 4s..4s+3 = W[n][128j + 32s + 8kq ..+7]
    flat, sflat = lin.ft.reshape(-1), lin.scales.reshape(-1)
    for (n, k) in [(0, 0), (N - 1, K - 8), (N // 2, 136), (min(N - 1, 17), 360)]:
        nt, r, j, s, kq = n // 16, n % 16, k // 128, (k % 128) // 32, (k % 32) // 8
        off = ((nt * (K // 128) + j) * 64 + kq * 16 + r) * 16 + 4 * s
        assert torch.equal(flat[off: off + 4], c[n, k // 2: k // 2 + 4]), (n, k)
        assert int(sflat[((nt * (K // 128) + j) * 16 + r) * 4 + s]) == int(sc[n, k // 32]), (n, k)
    # rows beyond N are zero
    full_c, _ = ops.untile_mx_fp4(lin.ft, lin.scales, n16 * 16)
    assert not full_c[N:].any()


def test_k_constraint_is_stated():
    with pytest.raises(AssertionError, match="K % 512 == 0"):
        ops.PackedLinearW4(torch.zeros(16, 768))
