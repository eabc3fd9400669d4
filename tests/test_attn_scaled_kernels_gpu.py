"""mg_attn_prefill_scaled_bf16 (ABI 20; DESIGN.md "Explaining an answer"): causal flash attention with a per-key scale on the fp32
score,  s[t, j] = (q_t . k_j) / 16 * key_scale[b, j],  the causal mask applied AFTER the scaling.

  (a) key_scale == 1: the bits of mg_attn_prefill_bf16 under MAGMA_ATTN_FWD=5, the kernel it is built from;
  (b) per element against fp64 with the scale folded into the fp64 keys;
  (c) the running maximum is taken over the SCALED scores;
  (d) scale 0 everywhere: every row is the mean of the values it sees, lse = log(t + 1);
  (e) nothing is read past key_scale[b][S - 1];
  (f) the refusals, without a launch."""

import pytest
import torch

import kernel_compare as kcmp

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B, H = 2, 2
SIZES = (1, 33, 129, 290)     # one key / a ragged second tile / a second query block (its waves skip the mask on full tiles) / three
MG_ERR_SHAPE, MG_ERR_ALIGN = -1, -2


def rnd(*shape, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def operands(S, dev, seed=0):
    k = rnd(B, H, S, 256, dev=dev, seed=seed + 1, scale=0.5).to(BF16)
    v = rnd(B, H, S, 256, dev=dev, seed=seed + 2).to(BF16)
    q = rnd(B, H, S, 256, dev=dev, seed=seed + 3, scale=0.5).to(BF16)
    return q, k, v


def run_scaled(q, k, v, scale, S):
    from magma_amd import ops
    dev = q.device
    vt = ops.head_transpose(v, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    out = torch.full((B * S, H * 256), float("nan"), dtype=BF16, device=dev)
    lse = torch.full((B, H, S), float("nan"), dtype=torch.float32, device=dev)
    ops.attn_prefill_scaled(q, k, vt, out, B, H, S, scale, lse=lse)
    return out, lse


def run_plain(q, k, v, S):
    from magma_amd import ops
    dev = q.device
    vt = ops.head_transpose(v, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    out = torch.full((B * S, H * 256), float("nan"), dtype=BF16, device=dev)
    lse = torch.full((B, H, S), float("nan"), dtype=torch.float32, device=dev)
    ops.attn_prefill(q, k, vt, out, B, H, S, lse=lse)
    return out, lse


def scaled_terms(q, k, v, scale):
    """kernel_compare.attention_terms with the scale folded into the fp64 keys: the reference AND the magnitude products of the
    scaled scores."""
    S = q.shape[2]
    k64 = k.double() * scale.double()[:, None, :S, None]
    return kcmp.attention_terms(q, k64, v, kcmp.causal_mask(S, S, 0, q.device))


def scaled_bounds(terms, S, out_dtype=BF16, K=256):
    """kernel_compare.attention_bound / lse_bound, restated with ONE MORE rounding of the exponent: the multiply by the scale
    rounds the score once more, relative to |t_j| <= qk_mag_max (exp_rel_err counts K + 16 roundings at that magnitude: K + 17
    here).  Everything else is the unscaled kernel's arithmetic: bf16 P, one possible rescale per 32-key tile."""
    n_rescale = -(-S // 32)
    n_fp32 = S + S / 16 + 16
    e1 = kcmp.gamma(K + 17) * terms["qk_mag_max"] + kcmp.U_TRANS
    pv = terms["pv_mag"]
    err = kcmp.U_BF16 * pv + 2.0 * (e1 + n_rescale * kcmp.U_TRANS) * pv + 2.0 * kcmp.gamma(n_fp32) * pv
    out_bound = kcmp.rounded(terms["ref"], err, out_dtype)
    e = e1.squeeze(-1) + n_rescale * kcmp.U_TRANS + kcmp.gamma(n_fp32)
    mag = 2.0 * terms["qk_mag_max"].squeeze(-1) + terms["lse"].abs()
    lse_bound = e + (4.0 * kcmp.U_F32 + kcmp.U_TRANS) * (mag + 1.0) + kcmp.FLOOR
    return out_bound, lse_bound


def assert_scaled(out, lse, q, k, v, scale, what):
    S = q.shape[2]
    terms = scaled_terms(q, k, v, scale)
    ob, lb = scaled_bounds(terms, S)
    kcmp.assert_elementwise(out, kcmp.rows_of(terms["ref"]), kcmp.rows_of(ob), what)
    kcmp.assert_elementwise(lse, terms["lse"], lb, what + " (lse)")
    return terms, ob, lb


def scale_patterns(S, dev):
    g = torch.Generator().manual_seed(900 + S)
    yield "random in [0, 1]", torch.rand(B, S, generator=g).to(dev)
    for p in sorted({p for p in (0, 31, 32, 127, 128, S - 1) if p < S}):
        s = torch.ones(B, S)
        s[0, p] = 0.1
        s[1, (p + 1) % S] = 0.1        # the two batch rows carry different scales
        yield f"0.1 on key {p}", s.to(dev)
    s = torch.ones(B, S)
    s[0, S // 2] = 2.0
    s[1, S // 3] = 2.0
    yield "2.0 on one key", s.to(dev)


# ------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("S", SIZES)
def test_scale_one_has_the_bits_of_the_unscaled_kernel(dev, monkeypatch, S):
    monkeypatch.setenv("MAGMA_ATTN_FWD", "5")
    q, k, v = operands(S, dev, seed=10 * S)
    base, base_lse = run_plain(q, k, v, S)
    out, lse = run_scaled(q, k, v, torch.ones(B, S, device=dev), S)
    kcmp.assert_bit_exact(out, base.double(), f"scaled attention at scale 1, S={S}")
    kcmp.assert_bit_exact(lse, base_lse.double(), f"scaled attention at scale 1, S={S} (lse)")


# ------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("S", SIZES)
def test_scaled_attention_per_element(dev, S):
    q, k, v = operands(S, dev, seed=20 * S)
    for name, scale in scale_patterns(S, dev):
        out, lse = run_scaled(q, k, v, scale, S)
        assert_scaled(out, lse, q, k, v, scale, f"scaled attention S={S}, {name}")


# ------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("case", ("dominant key at 0.05", "strongly negative key at 0"))
def test_the_maximum_is_taken_after_scaling(dev, S, case):
    """The keys at the tile edges dominate their own query's row (raw score far above the rest: weights of the other keys
    underflow against a maximum over RAW scores once the dominant key is scaled down) -- or are as strongly negative and get
    scale 0, which puts them at score 0."""
    q, k, v = operands(S, dev, seed=30 * S)
    gain = 4.0 if case.startswith("dominant") else -4.0
    k = kcmp.dominant_edge_keys(q, k, gain=gain)
    idx = sorted({j for j in range(S) if j % 32 in (0, 31)} | {S - 1})
    scale = torch.ones(B, S)
    scale[0, idx] = 0.05 if gain > 0 else 0.0
    scale[1, idx[::2]] = 0.05 if gain > 0 else 0.0
    scale = scale.to(dev)
    out, lse = run_scaled(q, k, v, scale, S)
    assert_scaled(out, lse, q, k, v, scale, f"scaled attention S={S}, {case}")


# ------------------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("S", SIZES)
def test_scale_zero_everywhere_is_the_causal_mean(dev, S):
    q, k, v = operands(S, dev, seed=40 * S)
    scale = torch.zeros(B, S, device=dev)
    out, lse = run_scaled(q, k, v, scale, S)
    terms, ob, lb = assert_scaled(out, lse, q, k, v, scale, f"scaled attention S={S}, scale 0")
    n = torch.arange(1, S + 1, device=dev, dtype=torch.float64)
    mean = v.double().cumsum(2) / n[None, None, :, None]
    kcmp.assert_elementwise(out, kcmp.rows_of(mean), kcmp.rows_of(ob), f"scale 0, S={S}: the mean of v[0..t]")
    kcmp.assert_elementwise(lse, n.log()[None, None, :].expand(B, H, S).contiguous(), lb, f"scale 0, S={S}: lse = log(t + 1)")


# ------------------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("S", SIZES)
def test_nothing_is_read_past_the_last_scale(dev, S):
    q, k, v = operands(S, dev, seed=50 * S)
    g = torch.Generator().manual_seed(S)
    scale = torch.rand(B, S, generator=g).to(dev)
    out, lse = run_scaled(q, k, v, scale, S)
    wide = torch.full((B, S + 7), float("nan"), device=dev)
    wide[:, :S] = scale
    out_w, lse_w = run_scaled(q, k, v, wide[:, :S], S)       # row stride S + 7, NaN behind every row
    assert wide[:, :S].stride(0) == S + 7
    kcmp.assert_bit_exact(out_w, out.double(), f"ld_scale = S + 7, S={S}")
    kcmp.assert_bit_exact(lse_w, lse.double(), f"ld_scale = S + 7, S={S} (lse)")


# ------------------------------------------------------------------------------------------------------------ (f)
def test_launcher_refusals(dev):
    from magma_amd import lib, ops
    L = lib.load()
    S, Smax = 40, 64
    q, k, v = operands(Smax, dev, seed=7)
    q = q[:, :, :S].contiguous()
    vt = ops.head_transpose(v, B, H, Smax, sb=H * Smax * 256, ss=256, sh=Smax * 256)
    scale = torch.ones(B, S, device=dev)
    out = torch.full((B * S, H * 256), 7.0, dtype=BF16, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(qp=q.data_ptr(), kp=k.data_ptr(), vp=vt.data_ptr(), op=out.data_ptr(), ld_out=H * 256, Bn=B, Hn=H, Sn=S, Sm=Smax,
             vt_ld=Smax, sp=scale.data_ptr(), ld_scale=S):
        return L.mg_attn_prefill_scaled_bf16(qp, kp, vp, op, ld_out, None, Bn, Hn, Sn, Sm, vt_ld, sp, ld_scale, stream)

    assert call() == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    assert call(sp=None) == MG_ERR_SHAPE                      # null scale
    assert call(ld_scale=S - 1) == MG_ERR_SHAPE
    assert call(sp=scale.data_ptr() + 2) == MG_ERR_ALIGN
    assert call(Sn=4097, Sm=8192, vt_ld=4128, ld_scale=4097) == MG_ERR_SHAPE      # more scales than the LDS staging takes
    # ... and what mg_attn_prefill_bf16 refuses
    assert call(ld_out=H * 256 - 8) == MG_ERR_SHAPE
    assert call(ld_out=H * 256 + 2) == MG_ERR_SHAPE
    assert call(Bn=0) == MG_ERR_SHAPE
    assert call(Hn=0) == MG_ERR_SHAPE
    assert call(Sn=0) == MG_ERR_SHAPE
    assert call(Sn=Smax + 1, ld_scale=Smax + 1) == MG_ERR_SHAPE
    assert call(vt_ld=Smax + 8) == MG_ERR_SHAPE
    assert call(vt_ld=32) == MG_ERR_SHAPE
    for name in ("qp", "kp", "vp", "op"):
        assert call(**{name: None}) == MG_ERR_SHAPE, name
        assert call(**{name: {"qp": q, "kp": k, "vp": vt, "op": out}[name].data_ptr() + 8}) == MG_ERR_ALIGN, name
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call must not launch"
    assert b"mg_attn_prefill_scaled_bf16" in L.mg_last_error()


def test_ops_refusals(dev):
    from magma_amd import ops
    S = 40
    q, k, v = operands(S, dev, seed=8)
    vt = ops.head_transpose(v, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    out = torch.empty(B * S, H * 256, dtype=BF16, device=dev)
    ok = torch.ones(B, S, device=dev)
    ops.attn_prefill_scaled(q, k, vt, out, B, H, S, ok)
    for bad in (ok.double(), ok.to(BF16), ok[:, : S - 1], ok[:1], ok.view(-1), torch.ones(S, B, device=dev).t()):
        with pytest.raises(ValueError):
            ops.attn_prefill_scaled(q, k, vt, out, B, H, S, bad)
    with pytest.raises(ValueError):
        ops.attn_prefill_scaled(q.float(), k, vt, out, B, H, S, ok)
    with pytest.raises(ValueError):
        ops.attn_prefill_scaled(q[:, :, : S - 1], k, vt, out, B, H, S, ok)
    with pytest.raises(ValueError):
        ops.attn_prefill_scaled(q, k[:, :, : S - 1].contiguous(), vt, out, B, H, S, ok)
    with pytest.raises(ValueError):
        ops.attn_prefill_scaled(q, k, vt, out.float(), B, H, S, ok)
    with pytest.raises(ValueError):
        ops.attn_prefill_scaled(q, k, vt, out[: B * S - 1], B, H, S, ok)
    with pytest.raises(ValueError):
        ops.attn_prefill_scaled(q, k, vt, out, B, H, S, ok, lse=torch.empty(B, H, S, dtype=torch.float64, device=dev))
