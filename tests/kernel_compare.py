"""Per-element comparison of a kernel's output with an fp64 reference, against a bound DERIVED from the arithmetic the kernel does.

Why: the whole-tensor number of the suite (rel = ||got - ref||_F / ||ref||_F) averages.  A dropped 16-byte store at a tile corner,
a last row that reads the row above, a tail element without its bias all stay under its thresholds on a large tensor
(tests/test_kernel_compare_cpu.py keeps the figures).  Here every element has its own bound, and one element over it fails.

Conventions
    * inputs of the kernels are bf16 (or fp32) values, which fp64 holds exactly: references are formed in fp64 from them,
      on the device of the inputs (``f64``), so that a reference product is two extra matmuls and not a host round trip;
    * ``u`` is a unit roundoff: 2^-8 for bf16 (8 significand bits; ``f2bf`` / ``pack2bf`` in csrc/common.h round to nearest even),
      2^-24 for fp32.  ``gamma(n) = n u32 / (1 - n u32)`` is the standard bound on the relative error of n chained fp32 roundings
      (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).  A sum of K products accumulated in fp32 IN ANY ORDER has
      |computed - exact| <= gamma(K) * sum_k |a_k b_k|  (ibid. section 3.1: every term passes through at most K roundings whatever
      the tree), which is why one constructor covers split-K, both MFMA shapes, the GEMV bursts and wave reductions alike;
    * a value rounded once to the output type adds ``u_out |exact|``, and applies to the already perturbed value: the fp32 terms
      carry a factor (1 + u_out);
    * denormals: the MFMA and the packed conversions may flush them; an element then moves by less than 2^-126.  ``FLOOR`` (2^-120)
      covers a few dozen of those and is far below anything a test looks at.

None of the constants is fitted to what a kernel gives.  A ratio above 1 on the hardware is a finding: either a kernel fault (the
failure message shows where) or an error source missing here, which is then added as a NAMED term with its reason.

Plain module, imported by the tests the way fullwidth_common.py is: no fixtures, no pytest settings."""
import math

import torch

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -24
FLOOR = 2.0 ** -120
# hardware v_exp_f32 / v_log_f32 / v_rcp_f32 / v_rsq_f32: 1 ulp (CDNA ISA guide, "VOP1 transcendental precision") = 2 u32
U_TRANS = 2.0 * U_F32
# sup |d/dx gelu_new(x)| = 1.1290 (at x = 1.46): how far the tanh-form GELU stretches an error of its argument
GELU_LIPSCHITZ = 1.13
# CLIP's QuickGELU x sigmoid(1.702 x): the constant as the kernels hold it (1.702f, the fp32 value nearest to 1.702), and
# sup |d/dx| = 1.0998 (at 1.702 x = 2.40)
QUICK_GELU_K = 1.7020000219345093
QUICK_GELU_LIPSCHITZ = 1.10
# a plain fp32 division in device code: correctly rounded with hipcc's defaults; 2.5 ulp is what HIP / OpenCL state for the
# form a compiler may choose instead (-fno-hip-fp32-correctly-rounded-divide-sqrt).  2.5 ulp = 5 u32.
U_DIV = 5.0 * U_F32


def unit_roundoff(dtype) -> float:
    if dtype == torch.bfloat16:
        return U_BF16
    if dtype == torch.float32:
        return U_F32
    if dtype == torch.float64:
        return 2.0 ** -53
    raise ValueError(f"no unit roundoff for {dtype}")


def gamma(n: float) -> float:
    """n chained fp32 roundings: relative error <= n u / (1 - n u)."""
    nu = float(n) * U_F32
    assert nu < 0.5, "gamma(n) is meaningless for n u >= 1/2"
    return nu / (1.0 - nu)


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------------------------------------
def ratios(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """|got - ref| / bound per element (fp64); +inf where got is not finite although ref is."""
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    assert ref.dtype == torch.float64 and bound.dtype == torch.float64, "reference and bound are formed in fp64"
    g = f64(got)
    r = (g - ref).abs() / bound
    bad = ~torch.isfinite(g) & torch.isfinite(ref)
    return torch.where(bad | torch.isnan(r), torch.full_like(r, float("inf")), r)


def worst_ratio(got, ref, bound) -> float:
    return float(ratios(got, ref, bound).max()) if got.numel() else 0.0


def rel_l2(got, ref) -> float:
    """The whole-tensor number of the suite: kept in messages and as the second, coarser check of every test."""
    d = f64(got) - f64(ref)
    return float(d.norm() / (f64(ref).norm() + 1e-300))


def describe_failure(got, ref, bound, r=None) -> str:
    """Worst ratio and where, how many elements are over, and the bounding box of their indices -- a tile corner, one row,
    one 8-wide run look very different there."""
    r = ratios(got, ref, bound) if r is None else r
    over = r > 1.0
    n_over = int(over.sum())
    flat = int(torch.argmax(r))
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), r.shape)) if r.ndim else ()
    msg = (f"worst |err|/bound {float(r.reshape(-1)[flat]):.3g} at index {idx} "
           f"(got {float(f64(got).reshape(-1)[flat]):.9g}, ref {float(ref.reshape(-1)[flat]):.9g}, "
           f"bound {float(bound.reshape(-1)[flat]):.3g}); {n_over} of {r.numel()} elements over the bound")
    if n_over:
        nz = over.nonzero()
        lo, hi = nz.min(0).values.tolist(), nz.max(0).values.tolist()
        box = " x ".join(f"[{a}..{b}]" for a, b in zip(lo, hi))
        vol = 1
        for a, b in zip(lo, hi):
            vol *= b - a + 1
        msg += f"; bounding box of the offenders {box} ({n_over} of its {vol} elements)"
        nf = int((~torch.isfinite(f64(got)) & torch.isfinite(ref)).sum())
        if nf:
            msg += f"; {nf} not finite"
    return msg + f"; whole-tensor rel-L2 {rel_l2(got, ref):.3e}"


def assert_elementwise(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str = "") -> float:
    """Fails if any element has |got - ref| > bound or is not finite where ref is.  ref, bound: fp64, of got's shape.
    Prints (pytest -s / a log shows it) and returns the worst ratio of a passing comparison."""
    r = ratios(got, ref, bound)
    worst = float(r.max()) if r.numel() else 0.0
    print(f"[elementwise] {what}: worst err/bound {worst:.3g}, rel-L2 {rel_l2(got, ref):.3e}, {r.numel()} elements")
    assert worst <= 1.0, f"{what}: {describe_failure(got, ref, bound, r)}"
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# bound constructors
# ---------------------------------------------------------------------------------------------------------------------------
def rounded(ref: torch.Tensor, fp32_err: torch.Tensor, out_dtype) -> torch.Tensor:
    """A value computed in fp32 with absolute error <= fp32_err, then rounded ONCE to out_dtype:
    |fl(x + e) - x| <= u_out |x + e| + |e| <= u_out |x| + (1 + u_out) |e|."""
    u = unit_roundoff(out_dtype)
    return u * ref.abs() + (1.0 + u) * fp32_err + FLOOR


def product_terms(a: torch.Tensor, w: torch.Tensor):
    """(ref, mag) = (A W^T, |A| |W|^T) in fp64 on the operands' device -- the two extra products of a GEMM case."""
    a64, w64 = f64(a), f64(w)
    return a64 @ w64.t(), a64.abs() @ w64.abs().t()


def conv2d_terms(x: torch.Tensor, w: torch.Tensor, stride: int = 1, padding: int = 1):
    """(ref, mag, K) of a convolution as the GEMM it is run as: x [B, Cin, H, W], w [Cout, Cin, k, k] -> rows [B*Ho*Wo, Cout] in
    NHWC order; fp64 through unfold + matmul (no dependence on a vendor convolution in fp64)."""
    Cout, Cin, k, _ = w.shape
    cols = torch.nn.functional.unfold(f64(x), k, padding=padding, stride=stride)          # [B, Cin k k, Ho Wo]
    w2 = f64(w).reshape(Cout, Cin * k * k)
    to_rows = lambda t: t.permute(0, 2, 1).reshape(-1, Cout)
    return to_rows(w2 @ cols), to_rows(w2.abs() @ cols.abs()), Cin * k * k


# The scaled fp8 MFMAs -- v_mfma_scale_f32_16x16x128_f8f6f4 (the fp8 GEMMs) and v_mfma_scale_f32_32x32x64_f8f6f4 (the fp8 attention) --
# do not add their products the way an fp32 chain would.  Not in the ISA guide: measured on gfx950 one instruction at a time
# (mg_debug_mx_mfma / mg_debug_mx_mfma_acc), with powers of two, multi-bit and negative values, and the SAME for both forms:
#   1. Products are summed in groups of F8_MFMA*_GROUP = 8 consecutive k.  For the 32x32x64 form k = 32 b + 16 hi + r is byte
#      16 b + r of the lane in half-wave hi: a group is 8 consecutive bytes of ONE lane (one half of a 16-byte chunk); the other
#      half of the chunk, the lane's other chunk, the other half-wave and the other 32-block are other groups.  Inside a group
#      each product is aligned to the group's largest product and its bits below 2^-F8_MFMA*_KEEP_BITS = 2^-13 of that product's
#      leading bit are DROPPED (sign-magnitude truncation, no rounding: 2.1875 * 2^-2 beside 2^8 arrives as 2.125 * 2^-2,
#      -2^-6 beside 2^8 as 0).
#   2. The accumulator C does NOT take part in that alignment: a product of 2^-15 beside C = 2^8 (and of 2^-23 beside C = 1) arrives
#      exactly wherever it sits, and so does C = 2^-15 beside a product of 2^8.  C is added like one more group sum: the 8 (16)
#      group sums and C are aligned to the largest of them, and a term loses what lies more than F8_MFMA_SUM_BITS = 24 bits below
#      that one's leading bit -- one bit more than fp32 holds: two group sums of 2^-16 beside C = 2^8 add up to one ulp, four
#      (or eight) of 2^-17 are gone although they add up to one ulp (two); C = 1.5 * 2^-16 beside 2^8 is gone as well.  The sum is
#      rounded to nearest fp32 (C = 1.5 * 2^-15 beside 2^8 becomes 2^-14; a group sum of 2.1875 * 2^-17 becomes one ulp, 2^-15).
#      So the addition of C costs what an fp32 addition costs: per instruction each of the 9 (17) terms loses at most 2^-24 of
#      the largest and the sum rounds once, which the bounds count as 2 (K / 8 + 1) + 2 fp32 roundings relative to
#      |C| + sum |a_k w_k| (2 u32 per term, as the 16x16x128 test always did) -- inside gamma(K) for every chain here.
# tests/test_fp8_gpu.py::test_mx_mfma_sums_groups_of_8_and_truncates (16x16x128, C = 0), ::test_mx_mfma32_groups_and_truncation and
# ::test_mx_mfma_accumulator_rule pin all of it.
F8_MFMA_GROUP = 8
F8_MFMA_KEEP_BITS = 13
F8_MFMA32_GROUP = 8
F8_MFMA32_KEEP_BITS = 13
F8_MFMA_SUM_BITS = 24


def f8_mfma_truncation(a: torch.Tensor, w: torch.Tensor, group: int = F8_MFMA_GROUP, keep_bits: int = F8_MFMA_KEEP_BITS) -> torch.Tensor:
    """Named term of the fp8 paths: |error| of A W^T from the truncation inside the f8f6f4 MFMA.  In a group of 8 products the 7
    that are not the largest lose less than 2^-13 of the largest each, and |a_k w_k| <= max_g |a| max_g |w|:
        7 * 2^-13 * sum over groups g of  max_{k in g} |a_mk| * max_{k in g} |w_nk|        (one small matmul of group maxima).
    a, w: the DEQUANTISED operands [..., M, K], [..., N, K] in the instruction's k order (a group lies inside one 32-element scale
    block); group / keep_bits: the constants of the form that is used (F8_MFMA_* for 16x16x128, F8_MFMA32_* for 32x32x64)."""
    def gmax(t):
        t = f64(t).abs()
        pad = -t.shape[-1] % group
        if pad:
            t = torch.nn.functional.pad(t, (0, pad))
        return t.view(*t.shape[:-1], -1, group).amax(-1)
    return (group - 1) * 2.0 ** -keep_bits * (gmax(a) @ gmax(w).transpose(-1, -2))


def gemm_bound(ref, mag, K: int, out_dtype, *, n_epilogue: int = 0, bf16_partials: int = 0, act: str = "none",
               pre: torch.Tensor = None, extra_err: torch.Tensor = None) -> torch.Tensor:
    """out = round_out( act( sum_k a_k w_k [* scale] [+ bias] [+ residuals] ) ).

    ref          the exact OUTPUT (after the activation)
    mag          magnitude sum of every term that is added before the activation: |A| |W|^T [* |scale|] + |bias| + |res_0| + ...
    K            contraction length; n_epilogue = number of further fp32 operations of the epilogue (one per scale / bias / residual)
                 -> accumulation term gamma(K + n_epilogue) * mag, valid for any summation order (split-K slabs are fp32)
    bf16_partials  how many times a partial result is rounded to bf16 before it is combined (0 for every kernel of the library
                 today: split-K slabs and GEMV partials are fp32); each adds u_bf16 * mag
    act / pre    "none" | "relu" (1-Lipschitz: the bound passes through) | "gelu" (gelu_new_f of csrc/common.h:
                 x * rcp(1 + exp(-2u)), u = sqrt(2/pi) (x + 0.044715 x^3); ``pre`` = exact pre-activation).  The argument error is
                 stretched by at most GELU_LIPSCHITZ; the evaluation itself adds, relative to |gelu(x)|: the polynomial (4 roundings,
                 all terms of one sign) and the product with log2(e) move the exponent by (4 + 2) u32 |2u|, v_exp_f32 and
                 v_rcp_f32 are 1 ulp each, the add and the two multiplies one rounding each.
    extra_err    a further absolute error of the value before the activation (f8_mfma_truncation, scaled like the product)"""
    err = gamma(K + n_epilogue) * mag + bf16_partials * U_BF16 * mag
    if extra_err is not None:
        err = err + extra_err
    return rounded(ref, through_activation(err, act, pre, ref), out_dtype)


def through_activation(err, act: str, pre=None, ref=None):
    """The fp32 error of act(x) given the error ``err`` of x (see gemm_bound)."""
    if act == "gelu":
        assert pre is not None and ref is not None
        two_u = 2.0 * math.sqrt(2.0 / math.pi) * (pre + 0.044715 * pre ** 3)
        eval_rel = 6.0 * U_F32 * two_u.abs() + 2.0 * U_TRANS + 3.0 * U_F32
        return GELU_LIPSCHITZ * err + eval_rel * ref.abs()
    if act == "quick_gelu":
        # apply_act of csrc/common.h: v * __frcp_rn(1 + __expf(-1.702f v)).  The exponent t = 1.702 v is rounded as a product and
        # once more inside __expf (times log2 e): an absolute error 2 u32 |t| of the exponent is that relative error of the
        # exponential, which v_exp_f32 forms to 1 ulp; 1 + e inherits at most that relative error and rounds once, the reciprocal
        # is good to 1 ulp, the final product rounds once.
        assert pre is not None and ref is not None
        eval_rel = 2.0 * U_F32 * (QUICK_GELU_K * pre).abs() + 2.0 * U_TRANS + 2.0 * U_F32
        return QUICK_GELU_LIPSCHITZ * err + eval_rel * ref.abs()
    if act not in ("none", "relu"):
        raise ValueError(act)
    return err


def exp_rel_err(qk_mag_max: torch.Tensor, K: int) -> torch.Tensor:
    """Relative error of one softmax weight exp(t_j - m) as the kernels form it, t_j = (q . k_j) / 16:
       * the score is a K-term fp32 dot product: |dt| <= gamma(K) * (|q| . |k_j|) / 16;
       * scale, subtraction of the running maximum and the conversion to a base-2 exponent (an fma with 1/16 * log2(e), or a
         subtraction and __expf's multiply) round the exponent at most 4 times, each relative to a magnitude <= 2 max_j |t_j|;
         an absolute error d of the exponent is a relative error d of the exponential;
       * every later update of the running maximum multiplies the weight by exp(m_old - m_new): the exponents of those factors
         telescope to at most 2 max_j |t_j| in all, 4 more roundings at that magnitude (their hardware error: n_rescale below);
       * v_exp_f32 itself: 1 ulp.
    The SAME rounded maximum enters numerator and denominator of the softmax, so its own error cancels.
    qk_mag_max = max over the visible keys of (|q| . |k_j|) / 16, per query (broadcastable to the output)."""
    # K roundings at magnitude A = max (|q| . |k_j|) / 16, and 4 + 4 at magnitude 2 A = 16 at magnitude A
    return gamma(K + 16) * qk_mag_max + U_TRANS


def attention_terms(q, k, v, mask=None, scale: float = 1.0 / 16.0):
    """fp64 softmax(q k^T * scale) v with the magnitude products the bound needs.  q [..., Sq, D], k, v [..., Sk, D];
    mask (bool, broadcastable to [..., Sq, Sk]): True = visible.  -> dict(ref, pv_mag = P |V|, qk_mag_max [..., Sq, 1], lse, p)."""
    q64, k64, v64 = f64(q), f64(k), f64(v)
    t = q64 @ k64.transpose(-1, -2) * scale
    a = q64.abs() @ k64.abs().transpose(-1, -2) * scale
    if mask is not None:
        t = t.masked_fill(~mask, float("-inf"))
        a = a.masked_fill(~mask, 0.0)
    p = torch.softmax(t, -1)
    return dict(ref=p @ v64, pv_mag=p @ v64.abs(), qk_mag_max=a.max(-1, keepdim=True).values, lse=torch.logsumexp(t, -1), p=p)


def attention_bound(terms: dict, n_keys: int, out_dtype=torch.bfloat16, *, K: int = 256, p_dtype=torch.bfloat16,
                    n_rescale: int = None, n_fp32: float = None) -> torch.Tensor:
    """o = round_out( (sum_j p~_j v_j) / (sum_j p_j) ),  p_j = exp(t_j - m).

    * p rounded to p_dtype before the PV product (bf16 on the MFMA in prefill / cached prefill / attn_fwd_rows; fp32, i.e. no
      such term, in decode attention and attn_small): u_p * (P |V|);
    * the exponential (exp_rel_err = e): numerator and denominator both move by a relative e: e * (P |V| + |ref|) <= 2 e P |V|;
      each of the n_rescale updates of the running maximum (default: one per 32-key tile; the kernels without tiles, decode
      attention with its single maximum and attn_small with one update per key at most, say so) is one more hardware
      exponential on every earlier weight: + n_rescale * U_TRANS;
    * fp32 accumulation of numerator (magnitude P |V|) and denominator (|ref| relative): n_fp32 roundings on the way of a term
      (default n_keys + n_keys / 16 + 16: the additions over n_keys keys, one multiply per tile for the rescale, cross-wave
      merges, reciprocal and final multiply): 2 * gamma(n_fp32) * P |V|;
    * output rounding: u_out |ref|."""
    if n_rescale is None:
        n_rescale = -(-n_keys // 32)
    if n_fp32 is None:
        n_fp32 = n_keys + n_keys / 16 + 16
    e = exp_rel_err(terms["qk_mag_max"], K) + n_rescale * U_TRANS
    u_p = unit_roundoff(p_dtype) if p_dtype != torch.float32 else 0.0
    pv = terms["pv_mag"]
    err = u_p * pv + 2.0 * e * pv + 2.0 * gamma(n_fp32) * pv
    return rounded(terms["ref"], err, out_dtype)


def lse_bound(terms: dict, n_keys: int, K: int = 256) -> torch.Tensor:
    """lse = m + log(sum_j exp(t_j - m)) in fp32: a relative error e of the sum is an absolute error e of its logarithm
    (exponential + accumulation); m, the logarithm (v_log_f32, 1 ulp, times ln 2) and the final add round relative to
    magnitudes <= 2 max |t| + |lse|."""
    e = exp_rel_err(terms["qk_mag_max"], K).squeeze(-1) + -(-n_keys // 32) * U_TRANS + gamma(n_keys + n_keys / 16 + 16)
    mag = 2.0 * terms["qk_mag_max"].squeeze(-1) + terms["lse"].abs()
    return e + (4.0 * U_F32 + U_TRANS) * (mag + 1.0) + FLOOR


def layernorm_terms(x, g, b, eps: float):
    x64, g64, b64 = f64(x), f64(g), f64(b)
    mean = x64.mean(-1, keepdim=True)
    xc = x64 - mean
    var = (xc * xc).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    return dict(ref=xc * rstd * g64 + b64, mean=mean, var=var, rstd=rstd, xc=xc, x=x64, g=g64, b=b64, eps=eps)


def layernorm_bound(t: dict, d: int, out_dtype=torch.bfloat16, *, one_pass_variance: bool = False) -> torch.Tensor:
    """y = round_out( (x - mean) * rstd * g + b ), statistics by fp32 row reductions over d terms.

    * mean: |d mean| <= gamma(d + 1) * mean|x|;
    * variance, two-pass form sum (x - mean)^2 / d: relative gamma(d + 4), plus 2 |d mean| mean|x - mean| / var ... bounded below
      through the Cauchy-Schwarz step mean|x - mean| <= sqrt(var);  one-pass form E[x^2] - mean^2 (one_pass_variance): the
      cancellation costs gamma(d + 4) * (E[x^2] + mean^2) / var instead;
    * rstd = rsq(var + eps): half the relative error of var, + 1 ulp;
    * the element: (x - mean) carries |d mean| + u32 |x - mean|; three more roundings for * rstd, * g, + b."""
    x, xc, var, rstd, g, b = t["x"], t["xc"], t["var"], t["rstd"], t["g"], t["b"]
    mean_abs = x.abs().mean(-1, keepdim=True)
    d_mean = gamma(d + 1) * mean_abs
    ve = var + t["eps"]
    if one_pass_variance:
        ex2 = (x * x).mean(-1, keepdim=True)
        d_var = gamma(d + 4) * (ex2 + t["mean"] ** 2) + 2.0 * t["mean"].abs() * d_mean
    else:
        d_var = gamma(d + 4) * var + 2.0 * d_mean * var.sqrt() + d_mean ** 2
    rel_rstd = 0.5 * d_var / ve + U_TRANS + U_F32
    scale = (rstd * g).abs()
    err = scale * (d_mean + U_F32 * xc.abs()) + (xc * rstd * g).abs() * (rel_rstd + 3.0 * U_F32) + U_F32 * (t["ref"].abs() + b.abs())
    return rounded(t["ref"], err, out_dtype)


def map_bound(ref: torch.Tensor, mag: torch.Tensor, n_ops: int, out_dtype) -> torch.Tensor:
    """An element-wise map of n_ops fp32 operations on terms whose magnitudes add up to ``mag`` (no reduction)."""
    return rounded(ref, gamma(n_ops) * mag, out_dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs that make the boundaries count
# ---------------------------------------------------------------------------------------------------------------------------
def self_dominant_qkv(shape, c: float, seed: int, device="cpu"):
    """q of scale 0.5, k_i = bf16(c q_i + 0.25 noise), v of scale 1 (bf16 tensors of ``shape`` = [..., S, D]): each query's own
    key dominates its softmax row (t_ii ~ c |q_i|^2 / 16 = 4 c at D = 256 against a spread of ~1 for the others), so a causal
    boundary that is off by one -- the diagonal key left out, a row that reads the row above -- changes the output by far more
    than the bound.  With i.i.d. q / k / v a long row averages ~S values and one missing key is invisible to any comparator."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(*shape, generator=g) * 0.5).to(torch.bfloat16)
    k = (c * q.float() + 0.25 * torch.randn(*shape, generator=g)).to(torch.bfloat16)
    v = torch.randn(*shape, generator=g).to(torch.bfloat16)
    return q.to(device), k.to(device), v.to(device)


# ---------------------------------------------------------------------------------------------------------------------------
# one-call forms for the GEMM / GEMV tests
# ---------------------------------------------------------------------------------------------------------------------------
def gelu_new64(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def linear_reference(a=None, w=None, *, prod=None, bias=None, scale=None, row_scale=None, residuals=(), base=None, act: str = "none",
                     act_n0: int = 0, post_residuals=(), out_dtype=torch.bfloat16, bf16_partials: int = 0):
    """(ref, bound) of  out = [base +] act( (A W^T) [* scale[n]] [* row_scale[m]] [+ bias[n]] [+ residuals] ) [+ post_residuals],
    the activation on the columns >= act_n0, everything in fp64 on the operands' device.  ``prod`` = (exact product, magnitude
    product, K [, a further absolute error of the product]) replaces A, W for operands that are not plain matrices (the
    implicit-im2col convolution) or whose product carries a named term of its own (the fp8 MFMA)."""
    extra = None
    if prod is None:
        p, m = product_terms(a, w)
        K = a.shape[1]
    elif len(prod) == 4:
        p, m, K, extra = prod
    else:
        p, m, K = prod
    n = 0
    if scale is not None:
        p, m, n = p * f64(scale), m * f64(scale).abs(), n + 1
        extra = None if extra is None else extra * f64(scale).abs()
    if row_scale is not None:
        p, m, n = p * f64(row_scale)[:, None], m * f64(row_scale).abs()[:, None], n + 1
        extra = None if extra is None else extra * f64(row_scale).abs()[:, None]
    if bias is not None:
        p, m, n = p + f64(bias), m + f64(bias).abs(), n + 1
    for r in residuals:
        p, m, n = p + f64(r), m + f64(r).abs(), n + 1
    if base is not None:
        assert act == "none"
        p, m, n = p + f64(base), m + f64(base).abs(), n + 1
    pre = p
    if act == "relu":
        ref = torch.relu(pre)
    elif act == "gelu":
        ref = gelu_new64(pre)
    else:
        ref = pre
    if act_n0:
        col = torch.arange(pre.shape[1], device=pre.device) >= act_n0
        ref = torch.where(col, ref, pre)
    if not post_residuals:
        bound = gemm_bound(ref, m, K, out_dtype, n_epilogue=n, bf16_partials=bf16_partials, act=act, pre=pre, extra_err=extra)
        if act_n0 and act == "gelu":
            bound = torch.where(col, bound, gemm_bound(pre, m, K, out_dtype, n_epilogue=n, bf16_partials=bf16_partials, extra_err=extra))
        return ref, bound
    # terms added after the activation: the activation's fp32 error (the bound of an fp32 output less its own rounding)
    # passes through, each addition rounds once relative to the magnitudes added so far
    act_err = gemm_bound(ref, m, K, torch.float64, n_epilogue=n, bf16_partials=bf16_partials, act=act, pre=pre, extra_err=extra)
    if act_n0 and act == "gelu":
        act_err = torch.where(col, act_err, gemm_bound(pre, m, K, torch.float64, n_epilogue=n, bf16_partials=bf16_partials, extra_err=extra))
    out, mag = ref, ref.abs()
    for r in post_residuals:
        out, mag = out + f64(r), mag + f64(r).abs()
    return out, rounded(out, act_err + gamma(len(post_residuals)) * mag, out_dtype)


ACTS = ("none", "relu", "gelu", "quick_gelu")
AUX_MODES = ("none", "relu_gate", "gelu_grad", "mul", "quick_gelu_grad")


def aux_factor_terms(aux: torch.Tensor, aux_mode: str):
    """(f, d_f): the factor an aux mode makes of the bf16 aux operand (exact in fp64) and the fp32 error of forming it.
    relu_gate is ``aux > 0`` exactly as the kernels write it: 0.0 and -0.0 close the gate."""
    a = f64(aux)
    if aux_mode == "relu_gate":
        return (a > 0).to(torch.float64), torch.zeros_like(a)
    if aux_mode == "mul":
        return a, torch.zeros_like(a)
    if aux_mode == "gelu_grad":
        return gelu_new_grad_terms(a)
    if aux_mode == "quick_gelu_grad":
        return quick_gelu_grad_terms(a)
    raise ValueError(aux_mode)


def epilogue_reference(prod_terms, *, scale=None, row_scale=None, bias=None, act: str = "none", act_n0: int = 0, aux=None,
                       aux_mode: str = "none", aux_after: bool = False, residuals=(), act_after: str = "none", base=None,
                       out_dtype=torch.bfloat16) -> dict:
    """The contract of mg_epilogue (include/magma_hip.h), literally and in its order, in fp64 with per-element bounds:

        v = (acc * row_scale[m]) * scale[n] + bias[n];   C2 = bf16(v);   v = act(v) on the columns >= act_n0;
        v *= f(aux) unless aux_after;   v += res0;  v += res1;  v += res2;   v *= f(aux) if aux_after;
        v = relu(v) if act_after;   C = out_dtype(v), or C = base + v (fp32, ``accumulate``)
        -> {"C": (ref, bound), "C2": (ref, bound)}

    prod_terms = (exact product, magnitude product, K [, a further absolute error of the product]) as product_terms /
    conv2d_terms / the fp8 tests' dequantised_product give it.  act: one of ACTS; aux_mode: one of AUX_MODES.

    The bound carries the pair (exact value x, fp32 error e) through the same steps.  One fp32 operation on a value with error
    e gives |fl(x~) - x| <= e + u32 (|x| + e) (``once``); a product with an exact factor s multiplies e by |s| first.
      accumulator   e = gamma(K) * mag [+ the product's own term]: K products summed in fp32 in any order
      row_scale, scale, bias, each residual, base: one operation each (the kernels may contract scale and bias into one fma:
                    fewer roundings, never more)
      C2            one rounding of (x, e) to bf16
      act           through_activation: relu 1-Lipschitz; gelu / quick_gelu stretch e by their Lipschitz constant and add the
                    evaluation error; columns < act_n0 keep (x, e)
      aux product   x f with |f~ - f| <= d_f (aux_factor_terms; 0 for the gate and the plain product): e |f| + (|x| + e) d_f, one
                    more rounding.  With aux_after the pair that is multiplied already holds the residual sum, so the factor
                    applies to the residuals' roundings too -- and a closed gate makes the output exactly 0
      act_after     ReLU is 1-Lipschitz: x = relu(x), e unchanged
      store         ``rounded``: u_out |x| + (1 + u_out) e"""
    if len(prod_terms) == 4:
        x, mag, K, extra = prod_terms
    else:
        (x, mag, K), extra = prod_terms, None
    assert act in ACTS and aux_mode in AUX_MODES and act_after in ("none", "relu")
    e = gamma(K) * mag
    if extra is not None:
        e = e + extra

    def once(x, e):
        return e + U_F32 * (x.abs() + e)

    if row_scale is not None:
        s = f64(row_scale)[:, None]
        x, e = x * s, e * s.abs()
        e = once(x, e)
    if scale is not None:
        s = f64(scale)
        x, e = x * s, e * s.abs()
        e = once(x, e)
    if bias is not None:
        x = x + f64(bias)
        e = once(x, e)
    out = {"C2": (x, rounded(x, e, torch.bfloat16))}
    if act != "none":
        y = torch.relu(x) if act == "relu" else (gelu_new64(x) if act == "gelu" else quick_gelu64(x))
        ye = through_activation(e, act, x, y)
        if act_n0:
            col = torch.arange(x.shape[1], device=x.device) >= act_n0
            y, ye = torch.where(col, y, x), torch.where(col, ye, e)
        x, e = y, ye
    if aux_mode != "none":
        f, d_f = aux_factor_terms(aux, aux_mode)

    def times_aux(x, e):
        xe = e * f.abs() + (x.abs() + e) * d_f
        x = x * f
        return x, once(x, xe)

    if aux_mode != "none" and not aux_after:
        x, e = times_aux(x, e)
    for r in residuals:
        x = x + f64(r)
        e = once(x, e)
    if aux_mode != "none" and aux_after:
        x, e = times_aux(x, e)
    if act_after == "relu":
        x = torch.relu(x)
    if base is not None:
        assert out_dtype == torch.float32, "accumulate adds into an fp32 output"
        x = x + f64(base)
        e = once(x, e)
    out["C"] = (x, rounded(x, e, out_dtype))
    return out


def assert_linear(out: torch.Tensor, what: str, a=None, w=None, **kw) -> float:
    """Per-element check of a GEMM / GEMV output against linear_reference(...) of the same operands (out_dtype = out's)."""
    ref, bound = linear_reference(a, w, out_dtype=out.dtype, **kw)
    return assert_elementwise(out, ref, bound, what)


# ---------------------------------------------------------------------------------------------------------------------------
# one-call forms for the attention tests
# ---------------------------------------------------------------------------------------------------------------------------
def causal_mask(Sq: int, Sk: int, p0, device) -> torch.Tensor:
    """[.., Sq, Sk] bool: query t (at position p0 + t) sees keys 0 .. p0 + t.  p0: int, or a tensor [B] of per-row positions
    (-> [B, 1, Sq, Sk])."""
    key = torch.arange(Sk, device=device)[None, :]
    qpos = torch.arange(Sq, device=device)[:, None]
    if torch.is_tensor(p0):
        return key[None, None] <= (qpos[None, None] + p0.to(device).view(-1, 1, 1, 1))
    return key <= qpos + p0


def rows_of(t: torch.Tensor) -> torch.Tensor:
    """[B, H, S, D] -> the [B*S, H*D] activation layout the attention kernels write."""
    B, H, S, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, H * D)


def assert_causal_attention(out_rows, q, k, v, what: str, *, p0=0, p_dtype=torch.bfloat16, lse=None, n_rescale: int = None) -> float:
    """out_rows [B*Sq, H*D] (any row stride) = softmax(q k^T / 16 under the causal mask at offset p0) v, per element against
    attention_bound; q [B, H, Sq, D], k / v [B, H, Sk, D] with Sk >= p0 + Sq.  lse [B, H, Sq] fp32 is checked too when given.
    n_rescale: see attention_bound (0 for the decode kernels, which take one maximum before any exponential)."""
    Sq, Sk = q.shape[2], k.shape[2]
    T = attention_terms(q, k, v, causal_mask(Sq, Sk, p0, q.device))
    n_keys = int(p0.max()) + Sq if torch.is_tensor(p0) else p0 + Sq
    bound = attention_bound(T, n_keys, out_rows.dtype, K=q.shape[-1], p_dtype=p_dtype, n_rescale=n_rescale)
    worst = assert_elementwise(out_rows, rows_of(T["ref"]), rows_of(bound), what)
    if lse is not None:
        assert_elementwise(lse, T["lse"], lse_bound(T, n_keys, K=q.shape[-1]), what + " (lse)")
    return worst


def dominant_edge_keys(q: torch.Tensor, k: torch.Tensor, gain: float = 4.0, tile: int = 32) -> torch.Tensor:
    """k with the keys at the edges of the kernels' 32-key tiles (first and last key of every tile, and the very last key, which
    ends a PARTIAL tile when S % 32 != 0) replaced by bf16(gain * q) of the same position: each of those keys dominates the row of
    its own query, the only one that sees it as its newest key -- a causal limit or a tile tail that is off by one there shows."""
    S = k.shape[-2]
    idx = sorted({j for j in range(S) if j % tile in (0, tile - 1)} | {S - 1})
    k = k.clone()
    k[..., idx, :] = (q[..., idx, :].float() * gain).to(torch.bfloat16)
    return k


# ---------------------------------------------------------------------------------------------------------------------------
# the fp8 attention forward (csrc/attention_fwd32_fp8.hip)
# ---------------------------------------------------------------------------------------------------------------------------
FP8_ATTN_TILE = 64          # keys per tile of the kernel: one PV instruction, one possible update of the deferred maximum
FP8_ATTN_DEFER = 4.0        # P_DEFER: the maximum moves only when a tile's maximum exceeds it by more than this (log2 units)
FP8_ATTN_INPUTS = ("self c=1", "self c=2", "tile edges", "next key")


def fp8_attn_key_order() -> list:
    """The keys of a 64-key tile in the k order of the PV instruction: k = 32 b + 16 hi + r (byte 16 b + r of a lane of half-wave
    hi, see the F8_MFMA32_* comment) holds key 32 b + (r & 3) + 8 (r >> 2) + 4 hi (the header of attention_fwd32_fp8.hip)."""
    return [32 * b + (r & 3) + 8 * (r >> 2) + 4 * hi for b in range(2) for hi in range(2) for r in range(16)]


def fp8_attention_inputs(kind: str, shape, seed: int, device="cpu", rot_dim: int = 64):
    """(q, k, v) bf16 [..., S, D] BEFORE the rotary, for which one boundary of the fp8 attention kernel each decides the output:
      "self c=1" / "self c=2"   self_dominant_qkv: a query's own key dominates -- the causal limit one too low, a wrong V byte or
                    V scale under the newest key; with c = 2 the row maximum jumps by more than the deferral threshold at the
                    newest key (a rescale that must reach everything accumulated before);
      "tile edges"  dominant_edge_keys, gain 4, on i.i.d. q / k of scale 0.5: only the first / last key of each 32-key block;
      "next key"    k[i + 1] = bf16(2 q[i] + 0.25 noise) in the dimensions >= rot_dim (noise alone below: the rotary turns
                    positions i and i + 1 by different angles there), q of scale 0.5: the key one PAST the causal limit would
                    dominate the row, so a limit one too high shows.  Nothing in the other kinds makes a future key matter.
    q and k of one position get the same rotation, so k[i] = c q[i] survives it.
    v is N(0, 1) times a power of two 2^-2 .. 2^2 drawn per (32 keys, d): neighbouring V^T blocks carry different E8M0 scales
    (with plain N(0, 1) every block's scale is 2^-7 and a scale taken from the wrong block is invisible)."""
    S, D = shape[-2], shape[-1]
    g = torch.Generator().manual_seed(seed + 1000)
    if kind.startswith("self c="):
        q, k, v = self_dominant_qkv(shape, float(kind[7:]), seed)
    else:
        q = (torch.randn(*shape, generator=g) * 0.5).to(torch.bfloat16)
        if kind == "tile edges":
            k = dominant_edge_keys(q, (torch.randn(*shape, generator=g) * 0.5).to(torch.bfloat16), gain=4.0, tile=32)
        elif kind == "next key":
            kf = 0.25 * torch.randn(*shape, generator=g)
            kf[..., 1:, rot_dim:] += 2.0 * q.float()[..., :-1, rot_dim:]
            k = kf.to(torch.bfloat16)
        else:
            raise ValueError(kind)
        v = torch.randn(*shape, generator=g).to(torch.bfloat16)
    gain = torch.exp2(torch.randint(-2, 3, (*shape[:-2], -(-S // 32), D), generator=g).float())
    v = (v.float() * gain.repeat_interleave(32, dim=-2)[..., :S, :]).to(torch.bfloat16)
    return q.to(device), k.to(device), v.to(device)


def qkv_rows(q, k, v) -> torch.Tensor:
    """q, k, v [B, H, S, D] -> the fused projection's output [B*S, 3*H*D] (columns: q | k | v, heads inside) the producers read."""
    B, H, S, D = q.shape
    return torch.stack([t.permute(0, 2, 1, 3) for t in (q, k, v)], 2).reshape(B * S, 3 * H * D).contiguous()


def fp8_attention_terms(q, k, v, mask) -> dict:
    """attention_terms on the DEQUANTISED operands + the three terms of fp8_attention_bound that need the operands themselves:
      qk_trunc [..., Sq, 1]   exponent error (nats) from the truncation inside the score MFMAs, the worst visible key of the row;
      p_round  [..., Sq, D]   P rounded to e4m3;      pv_trunc [..., Sq, D]   truncation inside the PV MFMAs."""
    T = attention_terms(q, k, v, mask)
    tr = f8_mfma_truncation(q, k, F8_MFMA32_GROUP, F8_MFMA32_KEEP_BITS) / 16.0
    T["qk_trunc"] = tr.masked_fill(~mask, 0.0).amax(-1, keepdim=True)
    del tr
    p, va = T["p"], f64(v).abs()
    pmax = p.amax(-1, keepdim=True)                           # = 1 / sum_j exp(t_j - max)
    e = p / pmax                                              # = exp(t_j - max)
    w = torch.where(e >= 2.0 ** -10, 2.0 ** -4 * p, torch.minimum(e, torch.full_like(e, 2.0 ** -14)) * pmax)
    T["p_round"] = w @ va
    del w, e
    Sk, G = k.shape[-2], F8_MFMA32_GROUP
    pad = -Sk % FP8_ATTN_TILE
    order = torch.tensor(fp8_attn_key_order(), device=p.device)
    idx = (torch.arange(0, Sk + pad, FP8_ATTN_TILE, device=p.device)[:, None] + order[None, :]).reshape(-1)
    gp = torch.nn.functional.pad(p, (0, pad))[..., idx]
    gp = gp.view(*gp.shape[:-1], -1, G).amax(-1)                                             # [..., Sq, groups]
    gv = torch.nn.functional.pad(va, (0, 0, 0, pad))[..., idx, :]
    gv = gv.view(*gv.shape[:-2], -1, G, gv.shape[-1]).amax(-2)                               # [..., groups, D]
    T["pv_trunc"] = (G - 1) * 2.0 ** -F8_MFMA32_KEEP_BITS * (1.0 + 2.0 ** -4) * (gp @ gv)
    return T


def fp8_attention_bound(terms: dict, n_keys: int, out_dtype=torch.bfloat16, *, K: int = 256) -> torch.Tensor:
    """o = round_out( (sum_j p~_j v_j) / (sum_j p_j) ) as mg_attn_prefill_fp8 forms it; ``terms`` = fp8_attention_terms of the
    dequantised operands (the values the kernel multiplies: their quantisation is the producer's business, not this bound's).

    Score.  t_j = (q . k_j) / 16 is four chained v_mfma_scale_f32_32x32x64_f8f6f4 (64 d each; a lane holds 32 consecutive d, so
      the instruction's groups are 8 consecutive d, and the per-token scales are common factors).  By the measured rule
      (F8_MFMA32_*) a product loses less than 2^-13 of the largest of its group: f8_mfma_truncation(q, k) / 16 = ``qk_trunc``, an
      ABSOLUTE error d of the exponent, i.e. a relative error expm1(d) of the weight.  The group sums and C are added at fp32
      width (F8_MFMA_SUM_BITS): 4 x 2 (8 + 1) = 72 roundings, fewer than the gamma(K) of exp_rel_err, which is kept as it is
      with the scale / maximum / exponential roundings it counts.
    Rescale.  The deferred maximum can move once per 64-key tile: n_rescale = ceil(n_keys / 64) hardware exponentials.
      All of the above is e; it moves numerator and denominator alike: 2 e P|V|.
    P rounded to e4m3 as 16 p.  The kernel's p_j = exp2(t_j - m2) is taken against the deferred maximum m2 of the moment, which
      only grows and stays within [running maximum - 4, running maximum] (P_DEFER), so 1 <= p_max <= 16 (16 p <= 256 < 448: no
      saturation) and every later rescale multiplies p~_j and the row sum by the same alpha.  e4m3 keeps 3 fraction bits: where
      16 p is normal (p >= 2^-10) the rounding is 2^-4 relative, and in output units 2^-4 softmax_j; below, it is at most
      min(p, 2^-14) absolute (half a subnormal step, or all of p), over a row sum lsum >= sum_j exp(t_j - max) because
      m2 <= max.  A key with exp(t_j - max) >= 2^-10 has p >= 2^-10 whatever m2 is; for the others both cases are below
      min(exp(t_j - max), 2^-14) / sum_j exp(t_j - max).  With the reference's own probabilities:
          p_round = sum_j |v_j| * ( 2^-4 softmax_j                                           if exp(t_j - max) >= 2^-10
                                    min(exp(t_j - max), 2^-14) / sum_i exp(t_i - max)        otherwise ),
      times (1 + e) because the rounded value already carries the exponential's error.  lsum adds the UNROUNDED p: the
      denominator has no such term.
    PV.  One instruction per tile: 64 keys in the order fp8_attn_key_order, V^T scaled per (d, 32 keys), P by 2^-4; groups of 8 in
      that order.  A product p~_j v_jd loses less than 2^-13 of the largest of its group, and tile, rescales and 1 / lsum scale
      a group's products alike:  pv_trunc = 7 * 2^-13 * (1 + 2^-4) * sum_groups max_g softmax_j * max_g |v_jd|.
      The running O enters as C: like one more group sum, at fp32 width -- 2 (8 + 1) roundings per 64 keys, inside n_fp32.
    The rest as in attention_bound: fp32 accumulation of numerator and denominator, n_fp32 = n_keys + n_keys / 16 + 16 roundings
      on the way of a term (additions, one multiply per tile for the rescale, the half-wave merge of lsum, reciprocal and final
      multiply), and the output rounding."""
    n_rescale = -(-n_keys // FP8_ATTN_TILE)
    e = exp_rel_err(terms["qk_mag_max"], K) + n_rescale * U_TRANS + torch.expm1(terms["qk_trunc"])
    pv = terms["pv_mag"]
    err = (1.0 + e) * terms["p_round"] + terms["pv_trunc"] + 2.0 * e * pv + 2.0 * gamma(n_keys + n_keys / 16 + 16) * pv
    return rounded(terms["ref"], err, out_dtype)


def fp8_lse_bound(terms: dict, n_keys: int, K: int = 256) -> torch.Tensor:
    """lse of the fp8 kernel: lse_bound + the exponent error of the score truncation (the worst key's bounds the logarithm of the
    sum).  P is summed unrounded: no e4m3 term."""
    return lse_bound(terms, n_keys, K) + terms["qk_trunc"].squeeze(-1)


def assert_causal_attention_fp8(out_rows, op, what: str, lse=None) -> float:
    """out_rows [B*S, H*256] (any row stride) of mg_attn_prefill_fp8 on ``op`` (ops.AttnFP8Operands), per element against
    fp8_attention_bound; the reference is fp64 causal attention on op.dequant().  lse [B, H, S] fp32 is checked when given."""
    q, k, v = op.dequant()
    S = q.shape[2]
    T = fp8_attention_terms(q, k, v, causal_mask(S, S, 0, q.device))
    worst = assert_elementwise(out_rows, rows_of(T["ref"]), rows_of(fp8_attention_bound(T, S, out_rows.dtype)), what)
    if lse is not None:
        assert_elementwise(lse, T["lse"], fp8_lse_bound(T, S), what + " (lse)")
    return worst


def deferred_maximum_trace(t2: torch.Tensor, visible: torch.Tensor, tile: int = FP8_ATTN_TILE, defer: float = FP8_ATTN_DEFER):
    """The deferred maximum of attention_fwd32_fp8.hip followed on exact scores: t2 [Sq, Sk] in log2 units, visible [Sq, Sk] bool.
    -> (moved, over): [Sq, tiles] bool -- the tile made the row's maximum move (a rescale of what was accumulated, after the
    first tile) / the tile's maximum lies above the kept one without moving it (its probabilities exceed 1)."""
    Sq, Sk = t2.shape
    m2 = torch.full((Sq,), -1e30, dtype=t2.dtype, device=t2.device)
    moved, over = [], []
    for s0 in range(0, Sk, tile):
        cand = t2[:, s0:s0 + tile].masked_fill(~visible[:, s0:s0 + tile], -1e30).amax(-1)
        up = cand > m2 + defer
        moved.append(up & (m2 > -1e29))
        over.append(~up & (cand > m2) & (cand > -1e29))
        m2 = torch.where(up, cand, m2)
    return torch.stack(moved, 1), torch.stack(over, 1)


def attention_backward_reference(q, k, v, dO_rows, out_rows, lse, *, p0: int = 0, scale: float = 1.0 / 16.0) -> dict:
    """What the flash-attention backward kernels compute FROM THEIR INPUTS -- q, k, v, the output gradient dO_rows [B*S, H*D] and the
    two tensors the forward kernel saved, out_rows (bf16 O, [B*S, H*D]) and lse (fp32, [B, H, S]) -- in fp64, with per-element
    bounds -> {"dq" | "dk" | "dv": (ref, bound)}, each [B, H, S, D] for bf16 outputs:

        P_ij = exp(q_i . k_j scale - lse_i),  D_i = sum_d dO_id O_id,  dS = P o (dO V^T - D),
        dV = P^T dO,  dQ = scale dS K,  dK = scale dS^T Q.

    The reference takes O and lse exactly as the backward kernel reads them.  The forward's own errors (a bf16 O, an lse that is
    a few ulp off) are the forward tests' business; taking D from the exact softmax instead would put sum_d |dO| bound(O) into
    every element of dQ and dK -- a worst case over 256 signed errors that is ~16 x what they add up to and hides a dropped store.

    What each step of the kernels (csrc/attention_bwd*.hip, attention_tr.hip) may add:
      P_ij  = exp2(s_ij sc2 - lse_i log2 e): the relative error e_p of a weight is that of the exponential (exp_rel_err) and the
              roundings of lse log2(e) and of the subtraction, relative to |lse|;
      dV_j  = sum_i bf16(P_ij) dO_i : (u_bf16 + e_p) per weight, fp32 accumulation over the queries;
      D_i   : an fp32 dot product over D terms;
      dS_ij = bf16( P_ij (dP_ij - D_i) ), dP = dO V^T an fp32 dot product over D; some variants multiply with the already rounded
              bf16(P) (two bf16 roundings), others with the fp32 weight: 2 u_bf16 covers both;
      dQ_i  = scale sum_j dS_ij k_j,  dK_j = scale sum_i dS_ij q_i : the error of dS passes through |K| / |Q|, + fp32 accumulation
              and the output rounding.

    "dq_err" | "dk_err" | "dv_err": the fp32 error terms alone, BEFORE the output rounding -- what an epilogue that does more
    than round (merged_backward_reference: the inverse rotary, then one rounding) has to carry on."""
    B, H, S, D = q.shape
    n_keys = p0 + S
    mask = causal_mask(S, k.shape[2], p0, q.device)
    q64, k64, v64 = f64(q), f64(k), f64(v)
    dO = f64(dO_rows).reshape(B, S, H, D).permute(0, 2, 1, 3)
    O = f64(out_rows).reshape(B, S, H, D).permute(0, 2, 1, 3)
    lse64 = f64(lse)[..., None]
    t = (q64 @ k64.transpose(-1, -2) * scale).masked_fill(~mask, float("-inf"))
    P = torch.exp(t - lse64)
    a_max = (q64.abs() @ k64.abs().transpose(-1, -2) * scale).masked_fill(~mask, 0.0).max(-1, keepdim=True).values
    u = U_BF16
    e_p = exp_rel_err(a_max, D) + 4.0 * U_F32 * (lse64.abs() + 1.0)                 # [B,H,S,1]
    dP, dP_mag = dO @ v64.transpose(-1, -2), dO.abs() @ v64.abs().transpose(-1, -2)
    Dv = (dO * O).sum(-1, keepdim=True)
    D_err = gamma(D + 8) * (dO.abs() * O.abs()).sum(-1, keepdim=True)
    dS = P * (dP - Dv)
    E = P * (gamma(D + 8) * dP_mag + D_err + gamma(2) * (dP.abs() + Dv.abs())) + (2.0 * u + e_p) * dS.abs()
    acc = gamma(n_keys + n_keys / 16 + 16)
    dV = P.transpose(-1, -2) @ dO
    dV_err = ((u + e_p) * P).transpose(-1, -2) @ dO.abs() + acc * (P.transpose(-1, -2) @ dO.abs())
    dQ = dS @ k64 * scale
    dQ_err = (E @ k64.abs() + acc * (dS.abs() @ k64.abs())) * scale
    dK = dS.transpose(-1, -2) @ q64 * scale
    dK_err = (E.transpose(-1, -2) @ q64.abs() + acc * (dS.abs().transpose(-1, -2) @ q64.abs())) * scale
    bf = torch.bfloat16
    return {"dq": (dQ, rounded(dQ, dQ_err, bf)), "dk": (dK, rounded(dK, dK_err, bf)), "dv": (dV, rounded(dV, dV_err, bf)),
            "dq_err": dQ_err, "dk_err": dK_err, "dv_err": dV_err}


def assert_attention_backward(dq, dk, dv, q, k, v, dO_rows, out_rows, lse, what: str) -> dict:
    ref = attention_backward_reference(q, k, v, dO_rows, out_rows, lse)
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert_elementwise(got, ref[name][0], ref[name][1], f"{what} {name}")
    return ref


MERGED_BWD_FAMILIES = ("i.i.d.", "self c=2")
MERGED_BWD_IID_SCALE = 1.5


def merged_backward_inputs(kind: str, B: int, H: int, S: int, seed: int = 50):
    """(q, k, v [B, H, S, 256], dO [B*S, H 256]) bf16 on the CPU for the tests of the merged backward, where ONE wrong row has to
    show in dq as well.  dq_i = sum_j dS_ij k_j / 16 is a sum of signed terms, and the bound follows their MAGNITUDES: under a flat
    softmax (i.i.d. q / k of scale 0.5: scores spread by 0.25) a row of n keys has |dq_i| ~ n^-1/2 of its magnitude sum, the bound
    is ~ 3 u_bf16 n^1/2 |dq_i|, and at n = 2048 no fault of a row's own size reaches 8 bounds.  Both families keep the softmax peaked:
      "i.i.d."     q, k ~ N(0, 1.5^2): scores spread by 1.5^2 = 2.25, the weights of a row are log-normal and a handful carry it
                   (n exp(-2.25^2) effective keys at most);
      "self c=2"   self_dominant_qkv with c = 2: a query's own key leads by ~8 and keeps more than half of the row at S = 2048
                   (c = 1 leads by 4 and is down to 3 % there).
    v and dO ~ N(0, 1).  tests/test_kernel_compare_cpu.py checks on the CPU that every seeded fault is >= 8 bounds for them.  That is
    a property of THESE draws, not of the families: dq stays the weak output (a turn by the neighbouring position's angles reaches
    9 .. 40 bounds in its last row at S = 2048 depending on the draw, a stronger lead, c = 3, makes rows one-hot and dq ~ 0), so
    the default seed is the one the CPU test was checked with."""
    g = torch.Generator().manual_seed(seed + 7 * S + H)
    if kind == "i.i.d.":
        q, k = ((torch.randn(B, H, S, 256, generator=g) * MERGED_BWD_IID_SCALE).to(torch.bfloat16) for _ in range(2))
        v = torch.randn(B, H, S, 256, generator=g).to(torch.bfloat16)
    elif kind.startswith("self c="):
        q, k, v = self_dominant_qkv((B, H, S, 256), float(kind[7:]), seed + 7 * S + H)
    else:
        raise ValueError(kind)
    return q, k, v, torch.randn(B * S, H * 256, generator=g).to(torch.bfloat16)


def inverse_rotary_with_error(x: torch.Tensor, err: torch.Tensor, sin_rows: torch.Tensor, cos_rows: torch.Tensor, rot_dim: int):
    """The inverse GPT-J turn R(-theta) of an fp64 value x [..., D] that a kernel holds in fp32 with absolute error <= err:
    y_2i = x_2i c + x_2i+1 s,  y_2i+1 = x_2i+1 c - x_2i s  on the first rot_dim columns -> (y, error of the fp32 y).
    Each element takes the error of itself through |c| and that of its pair partner through |s|; the arithmetic -- the 1/16 scale
    of the accumulator, two products, one addition: gamma(4) -- is relative to the magnitude sum of the two products as the
    kernel forms them (the perturbed values, hence |x| + err).  Columns >= rot_dim are not touched."""
    y, e = x.clone(), err.clone()
    if rot_dim == 0:
        return y, e
    s, c = f64(sin_rows).abs(), f64(cos_rows).abs()
    xe, xo, ee, eo = x[..., 0:rot_dim:2], x[..., 1:rot_dim:2], err[..., 0:rot_dim:2], err[..., 1:rot_dim:2]
    y[..., 0:rot_dim:2] = xe * f64(cos_rows) + xo * f64(sin_rows)
    y[..., 1:rot_dim:2] = xo * f64(cos_rows) - xe * f64(sin_rows)
    e[..., 0:rot_dim:2] = ee * c + eo * s + gamma(4) * ((xe.abs() + ee) * c + (xo.abs() + eo) * s)
    e[..., 1:rot_dim:2] = eo * c + ee * s + gamma(4) * ((xo.abs() + eo) * c + (xe.abs() + ee) * s)
    return y, e


def merged_backward_reference(ref: dict, sin_t, cos_t, rot_dim: int, B: int, H: int, S: int):
    """The MERGED output of the attention backward -- dqkv [B*S, 3 H 256] = [dq | dk | dv], the gradient of the fused qkv projection
    (mg_attn_bwd_merged_bf16, mg_attn_bwd_rows_bf16 with dqkv) -- from ``ref`` = attention_backward_reference(...) of the same
    operands -> (ref_rows, bound_rows), both [B*S, 3 H 256] fp64.

    The epilogues (store_grad_row, store_grad_tile32, store_grad_tile32_tr) turn the first rot_dim columns of every dq and dk head
    by R(-theta_s) with row s of the fp32 tables sin_t / cos_t [>= S, rot_dim / 2] (exact in fp64), in fp32, BEFORE the single
    rounding to bf16: inverse_rotary_with_error carries the un-rounded error terms of ``ref`` through the turn, ``rounded`` adds
    the one rounding.  Columns >= rot_dim and all of dv: the un-turned reference and error, i.e. the bound of the separate
    outputs.  Placement as grad_row_ptr (csrc/attn_bwd_device.h) states it: row b S + s, column which H 256 + h 256 + d."""
    ref_rows, bound_rows = [], []
    for name in ("dq", "dk", "dv"):
        x, err = ref[name][0], ref[name + "_err"]
        assert x.shape[0] == B and x.shape[1] == H and x.shape[2] == S, (x.shape, B, H, S)
        if name != "dv" and rot_dim:
            assert sin_t.shape[0] >= S and sin_t.shape[1] == rot_dim // 2 == cos_t.shape[1] and sin_t.dtype == torch.float32
            x, err = inverse_rotary_with_error(x, err, sin_t[:S].to(x.device), cos_t[:S].to(x.device), rot_dim)
        ref_rows.append(rows_of(x))
        bound_rows.append(rows_of(rounded(x, err, torch.bfloat16)))
    return torch.cat(ref_rows, 1), torch.cat(bound_rows, 1)


def assert_merged_attention_backward(dqkv, q, k, v, dO_rows, out_rows, lse, rot_dim: int, sin_t, cos_t, what: str, ref: dict = None) -> float:
    """dqkv [B*S, 3 H 256] per element against merged_backward_reference; ``ref``: the attention_backward_reference of the same
    operands where the caller has it already (assert_attention_backward returns it).  Returns the worst |err| / bound."""
    B, H, S, _ = q.shape
    if ref is None:
        ref = attention_backward_reference(q, k, v, dO_rows, out_rows, lse)
    ref_rows, bound_rows = merged_backward_reference(ref, sin_t, cos_t, rot_dim, B, H, S)
    return assert_elementwise(dqkv, ref_rows, bound_rows, what)


# ---------------------------------------------------------------------------------------------------------------------------
# the ViT attention backward (attn_small_bwd_kernel, csrc/elementwise.hip)
# ---------------------------------------------------------------------------------------------------------------------------
# (B, S, H): one token (dq = dk = 0, dv = dO); two tokens, two batch items, one head; a short odd sequence; ViT-B/32 at 224;
# one below the LDS limit; the limit with one head and with twelve; more workgroups (23 * 12 = 276) than the 256 CUs
ATTN_SMALL_BWD_SHAPES = ((1, 1, 3), (2, 2, 1), (1, 7, 2), (2, 50, 12), (2, 63, 2), (3, 64, 1), (1, 64, 12), (23, 50, 12))
ATTN_SMALL_BWD_FAMILIES = ("i.i.d.", "last key leads", "class rows only", "ViT scale")


def attn_small_lead_gain(S: int) -> float:
    """c of the "last key leads" family: the last key is c u, every query carries u (|u|^2 ~ 64), so that key's score is ~8 c
    above scores that spread by ~1.4.  0.75 from S = 7 on (a lead of 6: the median largest weight is 0.70 .. 0.91 against 50 .. 64
    rivals, 0.98 against 6), 0.5 (a lead of 4 over one rival: 0.98) below: peaked, but NOT one-hot -- a one-hot row has dS = 0
    exactly, and a dropped dq store is no fault there (tests/test_kernel_compare_cpu.py asserts both properties)."""
    return 0.75 if S >= 7 else 0.5


def attn_small_backward_inputs(family: str, B: int, S: int, H: int, seed: int = 731):
    """(qkv [B*S, 3*H*64], d_out [B*S, H*64]) bf16 on the CPU, from fixed seeds:
      "i.i.d."           unit Gaussians, as test_attn_small_forward;
      "last key leads"   that test's construction with the gain of attn_small_lead_gain: every row of P leans on column S - 1,
                         which an output sum that ends one index short leaves out;
      "class rows only"  d_out is zero except in row 0 of each image: what the last ViT block's backward is given (only the class
                         token is read); dP, dS and dq are then zero outside row 0;
      "ViT scale"        qkv * 0.7, unit d_out: the inputs of test_attn_small_backward."""
    g = torch.Generator().manual_seed(seed + 8 * S + H)
    w = H * 64
    qkv = torch.randn(B * S, 3 * w, generator=g)
    d_out = torch.randn(B * S, w, generator=g)
    if family == "ViT scale":
        qkv = qkv * 0.7
    elif family == "last key leads":
        u = torch.randn(1, 1, H, 64, generator=g)
        x = qkv.view(B, S, 3, H, 64)
        x[:, :, 0] += u
        if S > 1:
            x[:, S - 1, 1] = attn_small_lead_gain(S) * u[:, 0]
    elif family == "class rows only":
        d_out.view(B, S, w)[:, 1:] = 0.0
    elif family != "i.i.d.":
        raise ValueError(family)
    return qkv.to(torch.bfloat16), d_out.to(torch.bfloat16)


def heads_of(rows: torch.Tensor, B: int, S: int, H: int) -> torch.Tensor:
    """[B*S, n*H*64] rows (n = 3: the fused q | k | v columns; n = 1: one of them) -> [n, B, H, S, 64] views."""
    return rows.view(B, S, -1, H, 64).permute(2, 0, 3, 1, 4)


def attn_small_backward_reference(qkv, d_out, B: int, S: int, H: int) -> dict:
    """What mg_attn_small_bwd_bf16 computes from qkv [B*S, 3*H*64] and d_out [B*S, H*64], in fp64, with per-element bounds for its
    bf16 outputs -> {"dq" | "dk" | "dv": (ref, bound)}, each [B, H, S, 64]:

        t = q k^T / 8,  P = softmax(t),  dP = dO V^T,  D_i = sum_j P_ij dP_ij,  dS = P o (dP - D) / 8,
        dQ = dS K,  dK = dS^T Q,  dV = P^T dO.

    Unlike the flash kernels of attention_backward_reference this one saves nothing: everything is fp32 in LDS, nothing is masked,
    P is never rounded to bf16 and D comes from P o dP, not from an O of the forward.  One term per step of the kernel:
      score, dP   64-term fp32 dot products (the factor 1/8 is exact): gamma(64) (|q| . |k|) / 8 and gamma(64) (|dO| . |v|);
      P_ij        e = __expf(t_ij - m): exp_rel_err(max_j (|q| . |k_j|) / 8, 64) covers the score, the subtraction, __expf's own
                  multiply and v_exp_f32; the same rounded m enters numerator and denominator.  l adds S such terms in fp32
                  (each carries the exponential's error once more, and at most S roundings), inv = 1 / l is a division (U_DIV),
                  e * inv rounds once:  e_p = 2 exp_rel_err + gamma(S + 2) + U_DIV, relative;
      D_i         the sum of S products P~_ij dP~_ij in fp32:
                  sum_j P_ij (e_p |dP_ij| + gamma(64) (|dO| . |v|)_ij) + gamma(S) sum_j P_ij |dP_ij|;
      dS_ij       P~ (dP~ - D~) / 8, a subtraction and two products (the last by 1/8, exact -- counted all the same):
                  E_ij = P_ij (gamma(64) (|dO| . |v|)_ij + D_err_i + gamma(3) (|dP_ij| + |D_i|)) / 8 + (e_p + gamma(2)) |dS_ij|;
      dQ, dK, dV  sums over S terms in fp32: E |K| + gamma(S) |dS| |K|, its transposed form with |Q|, and
                  (e_p + gamma(S)) P^T |dO| with e_p of the row the weight comes from; then one rounding to bf16."""
    x = heads_of(f64(qkv), B, S, H)
    q, k, v = x[0], x[1], x[2]
    dO = heads_of(f64(d_out), B, S, H)[0]
    t = q @ k.transpose(-1, -2) * 0.125
    a_max = (q.abs() @ k.abs().transpose(-1, -2) * 0.125).max(-1, keepdim=True).values
    P = torch.softmax(t, -1)
    e_p = 2.0 * exp_rel_err(a_max, 64) + gamma(S + 2) + U_DIV                          # [B, H, S, 1]
    dP, dP_mag = dO @ v.transpose(-1, -2), dO.abs() @ v.abs().transpose(-1, -2)
    Dv = (P * dP).sum(-1, keepdim=True)
    D_err = (P * (e_p * dP.abs() + gamma(64) * dP_mag)).sum(-1, keepdim=True) + gamma(S) * (P * dP.abs()).sum(-1, keepdim=True)
    dS = P * (dP - Dv) * 0.125
    E = P * (gamma(64) * dP_mag + D_err + gamma(3) * (dP.abs() + Dv.abs())) * 0.125 + (e_p + gamma(2)) * dS.abs()
    acc = gamma(S)
    dQ = dS @ k
    dQ_err = E @ k.abs() + acc * (dS.abs() @ k.abs())
    dK = dS.transpose(-1, -2) @ q
    dK_err = E.transpose(-1, -2) @ q.abs() + acc * (dS.abs().transpose(-1, -2) @ q.abs())
    dV = P.transpose(-1, -2) @ dO
    dV_err = ((e_p + acc) * P).transpose(-1, -2) @ dO.abs()
    bf = torch.bfloat16
    return {"dq": (dQ, rounded(dQ, dQ_err, bf)), "dk": (dK, rounded(dK, dK_err, bf)), "dv": (dV, rounded(dV, dV_err, bf))}


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward, rotary, column sums
# ---------------------------------------------------------------------------------------------------------------------------
def layernorm_bwd_reference(dy, x, g, eps: float, res=None):
    """dx = rstd (gy - mean(gy) - xhat mean(gy xhat)) [+ res], gy = dy * g, and xhat, in fp64, with per-element bounds for bf16
    outputs -> {"dx": (ref, bound), "xhat": (ref, bound)}.

    The statistics are those of layernorm_bound (two-pass variance); xhat carries |rstd| (d_mean + u32 |x - mean|) and the
    relative error of rstd; the two row means are fp32 reductions over d terms (gamma(d + 3) of their magnitude sums), the second
    one also sees the error of xhat; the element combines three terms (gamma(4) of the magnitudes) and is scaled by rstd."""
    d = x.shape[-1]
    T = layernorm_terms(x, torch.ones(d, device=x.device), torch.zeros(d, device=x.device), eps)
    xc, var, rstd = T["xc"], T["var"], T["rstd"]
    xh = xc * rstd
    d_mean = gamma(d + 1) * T["x"].abs().mean(-1, keepdim=True)
    d_var = gamma(d + 4) * var + 2.0 * d_mean * var.sqrt() + d_mean ** 2
    rel_rstd = 0.5 * d_var / (var + eps) + U_TRANS + U_F32
    d_xh = rstd * (d_mean + U_F32 * xc.abs()) + xh.abs() * (rel_rstd + 2.0 * U_F32)
    gy = f64(dy) * f64(g)
    c1, c2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    d_c1 = gamma(d + 3) * gy.abs().mean(-1, keepdim=True)
    d_c2 = gamma(d + 4) * (gy * xh).abs().mean(-1, keepdim=True) + (gy.abs() * d_xh).mean(-1, keepdim=True)
    inner = gy - c1 - xh * c2
    inner_mag = gy.abs() + c1.abs() + (xh * c2).abs()
    d_inner = d_c1 + xh.abs() * d_c2 + c2.abs() * d_xh + gamma(4) * inner_mag
    dx = rstd * inner
    d_dx = rstd * d_inner + dx.abs() * (rel_rstd + U_F32)
    if res is not None:
        dx = dx + f64(res)
        d_dx = d_dx + U_F32 * (dx.abs() + f64(res).abs())
    bf = torch.bfloat16
    return {"dx": (dx, rounded(dx, d_dx, bf)), "xhat": (xh, rounded(xh, d_xh, bf))}


def rotary_reference(x: torch.Tensor, sin_rows: torch.Tensor, cos_rows: torch.Tensor, rot_dim: int, inverse: bool = False):
    """GPT-J rotary on the first rot_dim of the last axis, pairs (2 i, 2 i + 1) turned by angle i of the row's position:
    y_2i = x_2i c_i - x_2i+1 s_i,  y_2i+1 = x_2i+1 c_i + x_2i s_i.  x [..., D]; sin_rows / cos_rows [..., rot_dim / 2] (the fp32 table
    rows the kernel reads, broadcastable) -> (ref, bound): two products and one addition in fp32, one rounding to bf16.
    inverse: the turn back, y_2i = x_2i c_i + x_2i+1 s_i,  y_2i+1 = x_2i+1 c_i - x_2i s_i (what the backward applies to dq and dk)."""
    x64 = f64(x)
    s, c = f64(sin_rows), f64(cos_rows)
    if inverse:
        s = -s
    xe, xo = x64[..., 0:rot_dim:2], x64[..., 1:rot_dim:2]
    ref, mag = x64.clone(), x64.abs().clone()
    ref[..., 0:rot_dim:2], ref[..., 1:rot_dim:2] = xe * c - xo * s, xo * c + xe * s
    mag[..., 0:rot_dim:2] = mag[..., 1:rot_dim:2] = (xe * c).abs() + (xo * s).abs() + (xo * c).abs() + (xe * s).abs()
    err = gamma(2) * mag
    err[..., rot_dim:] = 0.0                 # copied, not computed
    return ref, rounded(ref, err, torch.bfloat16)


def ln_fold_reference(x, w2, b2, colsum, eps: float, act: str = "none", out_dtype=torch.bfloat16):
    """The decode GEMV with LayerNorm folded in (ops.fold_layernorm): y = act( rstd (x W'^T - mean colsum) + b' ) on the PRE-FOLDED
    operands (W' bf16, colsum and b' fp32 as given), mean / rstd of the row of x taken inside the kernel with the ONE-PASS variance
    E[x^2] - mean^2 -> (ref, bound).  The product: gamma(K) |x| |W'|^T; the mean: gamma(K + 2) mean|x|, multiplied by |colsum|;
    the variance cancels: gamma(K + 4) (E[x^2] + mean^2) + 2 |mean| d_mean, rstd inherits half of it relative to var + eps (+ v_rsq_f32);
    subtraction, two products and the bias: one rounding each relative to the magnitudes at hand."""
    K = x.shape[1]
    x64 = f64(x)
    P, Pmag = product_terms(x, w2)
    cs, b = f64(colsum), f64(b2)
    mean = x64.mean(-1, keepdim=True)
    ex2 = (x64 * x64).mean(-1, keepdim=True)
    var = (ex2 - mean ** 2).clamp_min(0)
    rstd = (var + eps).rsqrt()
    d_mean = gamma(K + 2) * x64.abs().mean(-1, keepdim=True)
    d_var = gamma(K + 4) * (ex2 + mean ** 2) + 2.0 * mean.abs() * d_mean
    rel_rstd = 0.5 * d_var / (var + eps) + U_TRANS + 2.0 * U_F32
    inner = P - mean * cs
    d_inner = gamma(K) * Pmag + cs.abs() * d_mean + gamma(2) * (P.abs() + (mean * cs).abs())
    pre = rstd * inner + b
    err = rstd * d_inner + (rstd * inner).abs() * (rel_rstd + U_F32) + U_F32 * (pre.abs() + b.abs())
    ref = gelu_new64(pre) if act == "gelu" else (torch.relu(pre) if act == "relu" else pre)
    return ref, rounded(ref, through_activation(err, act, pre, ref), out_dtype)


def cross_entropy_reference(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100) -> dict:
    """Row losses lse_r - logit_r[target] (0 on ignored rows), their mean over the valid rows and d mean-loss / d logits =
    (softmax - onehot) / n_valid (bf16), fp64, with bounds -> {"rows" | "mean" | "dlogits": (ref, bound), "n_valid", "n"}.

    The contract of the three kernels: a row is IGNORED when its target is ``ignore_index`` or lies outside [0, V) -- loss 0,
    gradient 0, not counted in n_valid (F.cross_entropy raises for such a target; the kernels cannot).  n = max(n_valid, 1);
    with n_valid = 0 the mean is NaN, as F.cross_entropy gives.

    A row reduction over V terms on 256 threads: the maximum is exact; every exponent logit - max is one rounding relative to at
    most 2 max|logit| and the libm exponential is good to 2 u32: e = 2 u32 (max|logit| + 1); the sum passes a term through at
    most V / 256 + 9 additions; reciprocal / logarithm (2 u32), the multiplications and the final additions one rounding each.
    The mean adds the R row losses in fp32 (all >= 0: gamma(R + 2) of the mean itself) and inherits the rows' own bounds."""
    lg = f64(logits)
    R, V = lg.shape
    tgl = targets.to(lg.device)
    valid = (tgl != ignore_index) & (tgl >= 0) & (tgl < V)
    n_valid = int(valid.sum())
    n = max(n_valid, 1)
    lmax = lg.abs().amax(-1, keepdim=True)
    e = 2.0 * U_F32 * (lmax + 1.0) + gamma(V / 256 + 16)
    lse = torch.logsumexp(lg, -1, keepdim=True)
    p = torch.exp(lg - lse)
    tg = torch.where(valid, tgl, torch.zeros_like(tgl))
    onehot = torch.zeros_like(lg).scatter_(1, tg[:, None], 1.0)
    v = valid[:, None]
    picked = lg.gather(1, tg[:, None])
    rows = torch.where(v, lse - picked, torch.zeros_like(lse)).squeeze(1)
    rows_err = torch.where(v, e + 4.0 * U_F32 * (lmax + lse.abs() + picked.abs() + 1.0), torch.zeros_like(lse)).squeeze(1)
    rows_bound = rounded(rows, rows_err, torch.float32)
    dl = torch.where(v, (p - onehot) / n, torch.zeros_like(p))
    dl_err = torch.where(v, (2.0 * e * p + 3.0 * U_F32 * (p + onehot)) / n, torch.zeros_like(p))
    mean = (rows.sum() / n_valid if n_valid else torch.full((), float("nan"), dtype=torch.float64, device=lg.device)).reshape(1)
    mean_bound = rounded(mean, (torch.where(valid, rows_bound, torch.zeros_like(rows_bound)).sum() / n).reshape(1)
                         + gamma(R + 2) * mean.abs(), torch.float32)
    return {"rows": (rows, rows_bound), "dlogits": (dl, rounded(dl, dl_err, torch.bfloat16)), "mean": (mean, mean_bound),
            "n": n, "n_valid": n_valid}


# ---------------------------------------------------------------------------------------------------------------------------
# inputs of the row kernels (LayerNorm, cross-entropy): the value families of tests/test_row_kernels_gpu.py, shared with the
# CPU checks of the bounds (tests/test_kernel_compare_cpu.py) so that both sides judge the same numbers
# ---------------------------------------------------------------------------------------------------------------------------
LN_FAMILIES = ("offset", "constant", "spike", "zero")


def layernorm_family_rows(kind: str, rows: int, d: int, seed: int) -> torch.Tensor:
    """bf16 [rows, d] on the CPU:
      "offset"    8 + 0.0625 N(0, 1): the mean is 128 standard deviations away, x - mean cancels 7 bits;
      "constant"  every element of row r the same bf16 value c_r (another one per row, both signs): variance 0,
                  rstd = eps^-1/2 multiplies whatever error the mean carries;
      "spike"     0.01 N(0, 1) with one element 200: at column 0 on even rows, at column d - 1 on odd rows;
      "zero"      all zero;
      "mixed"     row r of family r % 4 (spike rows alternate their column): neighbouring rows never share their statistics."""
    g = torch.Generator().manual_seed(seed)
    if kind == "offset":
        x = 8.0 + 0.0625 * torch.randn(rows, d, generator=g)
    elif kind == "constant":
        r = torch.arange(rows)
        c = (0.75 * (r % 5 + 1).float() + 0.0625 * (r % 3).float()) * (1.0 - 2.0 * (r % 2).float())
        x = c[:, None].expand(rows, d).clone()
    elif kind == "spike":
        x = 0.01 * torch.randn(rows, d, generator=g)
        r = torch.arange(rows)
        x[r, torch.where(r % 2 == 0, 0, d - 1)] = 200.0
    elif kind == "zero":
        x = torch.zeros(rows, d)
    elif kind == "mixed":
        x = torch.empty(rows, d)
        for i, fam in enumerate(LN_FAMILIES):
            n = len(range(i, rows, 4))
            if n:
                x[i::4] = layernorm_family_rows(fam, n, d, seed + 1 + i).float()
    else:
        raise ValueError(kind)
    return x.to(torch.bfloat16)


CE_FAMILIES = ("gauss", "peaked", "peaked off", "flat", "ignored", "underflow")


def cross_entropy_family(kind: str, R: int, V: int, seed: int):
    """(logits fp32 [R, V], targets int64 [R]) on the CPU:
      "gauss"       3 N(0, 1); targets of rows 0 .. 3 (as far as R goes): column 0, column V - 1, the row's arg-max column, and a
                    column whose logit is set to -200 (its probability underflows fp32); the other rows' targets are random;
      "peaked"      one logit +3e4 per row (column (7 r + 3) % V), the rest -3e4, target on the peak: loss and gradient exactly 0;
      "peaked off"  the same logits, target one column past the peak (mod V): loss 6e4, gradient +1/n at the peak and -1/n at
                    the target (V = 1 has no other column: target on the peak);
      "flat"        all logits 1e4: loss log V;
      "ignored"     "gauss" with every target -100;
      "underflow"   3 N(0, 1) with EVERY row's target logit set to -200 (its probability underflows fp32: the loss is ~200 + lse, the
                    gradient -1/n there); targets at column 0, at column V - 1 -- the last element of the tail pass of the
                    256-thread loops -- and, from row 2 on, random."""
    g = torch.Generator().manual_seed(seed)
    r = torch.arange(R)
    if kind in ("gauss", "ignored"):
        lg = 3.0 * torch.randn(R, V, generator=g)
        tg = torch.randint(0, V, (R,), generator=g)
        if R > 3:
            lg[3, V // 2] = -200.0
        k = min(R, 4)
        tg[:k] = torch.tensor([0, V - 1, int(lg[min(2, R - 1)].argmax()), V // 2])[:k]
        if kind == "ignored":
            tg[:] = -100
    elif kind == "underflow":
        lg = 3.0 * torch.randn(R, V, generator=g)
        tg = torch.randint(0, V, (R,), generator=g)
        tg[:min(R, 2)] = torch.tensor([0, V - 1])[:min(R, 2)]
        lg[r, tg] = -200.0
    elif kind in ("peaked", "peaked off"):
        peak = (7 * r + 3) % V
        lg = torch.full((R, V), -3e4)
        lg[r, peak] = 3e4
        tg = peak if kind == "peaked" else (peak + 1) % V
    elif kind == "flat":
        lg = torch.full((R, V), 1e4)
        tg = torch.randint(0, V, (R,), generator=g)
    else:
        raise ValueError(kind)
    return lg, tg.to(torch.int64)


def gelu_new_grad_terms(x: torch.Tensor):
    """d/dx gelu_new(x) as gelu_new_grad_f of csrc/common.h forms it -> (ref, fp32 error), fp64:
        sg = rcp(1 + exp(-2u)),  t = 2 sg - 1,  grad = sg + 0.5 x (1 - t^2) k0 (1 + 3 k1 x^2).
    sg has the relative error of gelu_new_f's sigmoid (through_activation); 1 - t^2 CANCELS for large |x|: its error is absolute,
    2 |t| d_t + 2 u32 with d_t = 2 d_sg + u32, and is multiplied by C = 0.5 |x| k0 (1 + 3 k1 x^2); the other factors and the final
    addition round once each relative to their magnitudes."""
    x = f64(x)
    k0, k1 = math.sqrt(2.0 / math.pi), 0.044715
    two_u = 2.0 * k0 * (x + k1 * x ** 3)
    sg = torch.sigmoid(two_u)
    t = 2.0 * sg - 1.0
    C = 0.5 * x.abs() * k0 * (1.0 + 3.0 * k1 * x * x)
    ref = sg + 0.5 * x * (1.0 - t * t) * k0 * (1.0 + 3.0 * k1 * x * x)
    d_sg = sg * (6.0 * U_F32 * two_u.abs() + 2.0 * U_TRANS + 2.0 * U_F32)
    d_t = 2.0 * d_sg + U_F32
    d_one_minus = 2.0 * t.abs() * d_t + 2.0 * U_F32
    err = d_sg + C * d_one_minus + gamma(8) * C * (1.0 - t * t) + U_F32 * (ref.abs() + sg)
    return ref, err


def quick_gelu64(x: torch.Tensor) -> torch.Tensor:
    return x * torch.sigmoid(QUICK_GELU_K * x)


def quick_gelu_grad_terms(x: torch.Tensor):
    """d/dx [x sigmoid(1.702 x)] as quick_gelu_grad_f of csrc/common.h forms it -> (ref, fp32 error), fp64:
        sg = 1 / (1 + exp(-t)), t = 1.702f x;      grad = sg * (1 + t (1 - sg)).
    sg = 1 / (1 + E): the exponent is rounded twice (the product, and __expf's own product with log2 e) -> 2 u32 |t| relative to the
    exponential E, v_exp_f32 1 ulp; a relative error d of E moves sg by sg (E / (1 + E)) d = sg (1 - sg) d; the addition rounds
    once, the division is good to U_DIV.  1 - sg CANCELS for large positive x (sg -> 1): its error is
    ABSOLUTE, d_sg + u32 (1 - sg), and is multiplied by |t|; t itself and the product t (1 - sg) round once each; 1 + (.) and the
    final product with sg round once each."""
    x = f64(x)
    t = QUICK_GELU_K * x
    sg = torch.sigmoid(t)
    om = torch.sigmoid(-t)                                  # 1 - sg without the cancellation
    d_sg = sg * (om * (2.0 * U_F32 * t.abs() + U_TRANS) + U_F32 + U_DIV)
    d_om = d_sg + U_F32 * om
    b = t * om
    d_b = t.abs() * d_om + 2.0 * U_F32 * b.abs()
    c = 1.0 + b
    d_c = d_b + U_F32 * c.abs()
    ref = sg * c
    err = c.abs() * d_sg + sg * d_c + U_F32 * ref.abs()
    return ref, err


# libm erff (OCML) has no accuracy statement in the HIP headers; OCML is built to the OpenCL full-profile table, which allows erf
# 16 ulp.  Named term of the two gelu_erf passes: 16 ulp = 32 u32 relative to |erf|.
ERFF_ULPS = 16


def gelu_erf_terms(x: torch.Tensor):
    """torch.nn.GELU() as gelu_erf_f / gelu_erf_grad_f of csrc/backward.hip form it -> (gelu, its fp32 error, gelu', its fp32 error):
        gelu = 0.5 x (1 + erf(z)), z = x / sqrt 2;      gelu' = 0.5 (1 + erf(z)) + x phi(x), phi = 0.39894 exp(-x^2 / 2) (__expf).
    1 + erf CANCELS for negative x: its error is absolute -- erff's ERFF_ULPS relative to |erf|, the rounding of z stretched by
    erf' = 2 / sqrt(pi) exp(-z^2), one addition; the exponential moves by (2 |y| + 4) u32 for the exponent y = x^2 / 2
    (two products, log2(e), v_exp_f32); every further product or addition rounds once."""
    x = f64(x)
    z = x / math.sqrt(2.0)
    erf = torch.erf(z)
    d_one_plus = (2.0 * ERFF_ULPS * U_F32 * erf.abs() + U_F32 * z.abs() * (2.0 / math.sqrt(math.pi)) * torch.exp(-z * z) * 2.0
                  + U_F32 * (1.0 + erf.abs()))
    gelu = 0.5 * x * (1.0 + erf)
    gelu_err = 0.5 * x.abs() * d_one_plus + 2.0 * U_F32 * gelu.abs()
    y = 0.5 * x * x
    xphi = x * 0.3989422804014327 * torch.exp(-y)
    grad = 0.5 * (1.0 + erf) + xphi
    grad_err = 0.5 * d_one_plus + xphi.abs() * ((2.0 * y + 4.0) * U_F32 + gamma(4)) + U_F32 * (grad.abs() + xphi.abs())
    return gelu, gelu_err, grad, grad_err


def adamw_reference(p0, m0, v0, g, norm_sq, lr, b1, b2, eps, wd, step: int, max_norm: float, grad_scale: float = 1.0) -> dict:
    """ONE step of the fused clip + AdamW kernel (csrc/backward.hip: adamw_kernel) from the state (p0, m0, v0), in fp64 on the same
    fp32 inputs and fp32-rounded hyper-parameters -> {"p" | "m" | "v": (ref, fp32 bound), "p_bf16": (ref, bf16 bound)}.
    The bias corrections 1 - beta^step cancel: their relative error is 3 u32 beta^step / (1 - beta^step) (powf to 2 ulp, one
    subtraction); the clip factor takes a square root, two products, an addition, a division and a minimum: gamma(8)."""
    f32c = lambda x: float(torch.tensor(x, dtype=torch.float32))
    lr, b1, b2, eps, wd, max_norm, gs = map(f32c, (lr, b1, b2, eps, wd, max_norm, grad_scale))
    d = f64
    clip = gs
    if norm_sq is not None and max_norm > 0:
        clip = gs * min(1.0, max_norm / (float(d(norm_sq).sqrt()) * gs + f32c(1e-6)))
    c_rel = gamma(8)
    gi = d(g) * clip
    m_r = b1 * d(m0) + (1 - b1) * gi
    d_m = gamma(4) * ((b1 * d(m0)).abs() + ((1 - b1) * gi).abs()) + (1 - b1) * gi.abs() * c_rel
    v_r = b2 * d(v0) + (1 - b2) * gi * gi
    d_v = gamma(5) * v_r + (1 - b2) * gi * gi * 2 * c_rel
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    rel_bc1, rel_bc2 = 3 * U_F32 * b1 ** step / bc1 + U_F32, 3 * U_F32 * b2 ** step / bc2 + U_F32
    p1 = d(p0) - lr * wd * d(p0)
    den = (v_r / bc2).sqrt() + eps
    upd = lr * (m_r / bc1) / den
    d_upd = lr / bc1 / den * d_m + upd.abs() * (rel_bc1 + 0.5 * (d_v / v_r.clamp_min(1e-300) + rel_bc2) + gamma(8))
    p_r = p1 - upd
    d_p = gamma(3) * (d(p0).abs() * (1 + lr * wd)) + d_upd + U_F32 * (p1.abs() + upd.abs())
    f32 = torch.float32
    return {"m": (m_r, rounded(m_r, d_m, f32)), "v": (v_r, rounded(v_r, d_v, f32)), "p": (p_r, rounded(p_r, d_p, f32)),
            "p_bf16": (p_r, rounded(p_r, d_p + U_F32 * p_r.abs(), torch.bfloat16))}


# ---------------------------------------------------------------------------------------------------------------------------
# gradient accumulation: a window against the sum of its micro-steps
# ---------------------------------------------------------------------------------------------------------------------------
ACC_ASSOC_ROUNDINGS = 8.0        # first term: 8 u32 of the magnitude sum
ACC_NOISE_FACTOR = 4.0           # second term: one repeat is ONE sample of the run-to-run noise
ACC_NOISE_FLOOR = 1e-5           # third term: the suite's figure for atomic noise (test_per_block_recompute_is_exact, test_dp_nccl_gpu.py)
ACC_VISIBLE = 100.0              # every part must be at least this many bounds large somewhere


def accumulation_reference(parts) -> torch.Tensor:
    """sum_i g_i in fp64: what a gradient buffer holds after a window whose micro-batches give g_1 .. g_N taken alone."""
    ref = f64(parts[0]).clone()
    for p in parts[1:]:
        ref += f64(p)
    return ref


def accumulation_bound(parts, repeats) -> torch.Tensor:
    """Per-element bound on |G - sum_i g_i| for ONE trainable tensor whose window gradient G accumulated N micro-steps.
    parts = [g_1 .. g_N]: the fp32 gradients of the micro-batches taken alone (each into a zeroed buffer); repeats: a second run
    of the same, [g_1' .. g_N'].

        8 u32 sum_i |g_i|  +  4 sum_i |g_i - g_i'|  +  1e-5 rms(sum_i g_i)

      * fp32 addition in another association (N - 1 additions of values the parts already rounded; every producer adds its
        K-term dot product to what the buffer holds instead of to zero), plus the one extra rounding an fma-style
        ``dst += s * src`` can have;
      * the run-to-run noise of the fp32 atomics behind the column sums, MEASURED reference against reference, never against the
        window; one repeat is a single sample of it, hence the factor;
      * a floor for the elements whose two samples happened to agree: the suite's own figure for that noise, as a fraction of the
        tensor's rms.
    FLOOR keeps the bound of a tensor that is exactly zero in every part positive (0 / 0 would read as a failure)."""
    assert len(parts) >= 1 and len(repeats) == len(parts)
    mag = torch.zeros_like(f64(parts[0]))
    noise = torch.zeros_like(mag)
    for p, r in zip(parts, repeats):
        mag += f64(p).abs()
        noise += (f64(p) - f64(r)).abs()
    ref = accumulation_reference(parts)
    rms = float(ref.pow(2).mean().sqrt()) if ref.numel() else 0.0
    return ACC_ASSOC_ROUNDINGS * U_F32 * mag + ACC_NOISE_FACTOR * noise + ACC_NOISE_FLOOR * rms + FLOOR


def accumulation_conditions(parts, repeats, what: str = ""):
    """The two conditions that hold BEFORE a window is looked at -> (ref, bound, self_ratio, invisible):

      1. reference within the bound: sum_i g_i' passes against sum_i g_i (asserted here; a failure says the bound is too tight
         for this tensor's noise, it does not blame the engine);
      2. every part is visible: max over the elements of |g_i| / bound >= ACC_VISIBLE for every i -- leaving part i out, or adding
         it twice, is then at least 100 bounds somewhere.  ``invisible`` lists (i, ratio, identically_zero) of the parts that
         are not; the caller decides (only an identically zero part may be excused)."""
    ref, bound = accumulation_reference(parts), accumulation_bound(parts, repeats)
    again = accumulation_reference(repeats)
    r = ratios(again, ref, bound)
    self_ratio = float(r.max()) if r.numel() else 0.0
    assert self_ratio <= 1.0, (f"{what}: the REFERENCE does not meet its own bound (a repeat of the parts against the first run): the "
                               f"bound is too tight for this tensor's run-to-run noise; {describe_failure(again, ref, bound, r)}")
    invisible = []
    for i, p in enumerate(parts):
        vis = float((f64(p).abs() / bound).max()) if ref.numel() else 0.0
        if vis < ACC_VISIBLE:
            invisible.append((i, vis, not bool(f64(p).any()) and not bool(f64(repeats[i]).any())))
    return ref, bound, self_ratio, invisible


def assert_accumulation(got, parts, repeats, what: str = "") -> dict:
    """One tensor of a window: both conditions, then got against sum_i g_i per element (assert_elementwise's report: worst
    ratio, index, count, bounding box).  A part that is not visible fails unless it is identically zero in both runs.
    -> {"worst", "self", "zero_parts"}."""
    ref, bound, self_ratio, invisible = accumulation_conditions(parts, repeats, what)
    bad = [(i, f"{v:.3g}") for i, v, zero in invisible if not zero]
    assert not bad, (f"{what}: part(s) {bad} (index, max |g_i| / bound) are below {ACC_VISIBLE:g}: a window that dropped them would "
                     f"pass.  Choose inputs under which every micro-batch moves this tensor; do not relax the condition")
    worst = assert_elementwise(got, ref, bound, what)
    return {"worst": worst, "self": self_ratio, "zero_parts": [i for i, _, zero in invisible if zero]}


# ---------------------------------------------------------------------------------------------------------------------------
# the NF-ResNet kernels (csrc/nfnet.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def f32_const(x: float) -> float:
    """A host double as the kernel receives it through a ``float`` argument."""
    return float(torch.tensor(x, dtype=torch.float32))


def _rsqrt_rel(d_ve, ve):
    """Relative error of rsqrtf(ve~) when |ve~ - ve| <= d_ve: (1 - x)^-1/2 - 1 <= x / (2 (1 - x)) for x = d_ve / ve in [0, 1)
    (the difference of the two sides is 0 at 0 and grows), then the hardware v_rsq_f32."""
    x = d_ve / ve
    assert float(x.max()) < 0.5, "the variance is not resolved in fp32: no bound to state"
    return 0.5 * x / (1.0 - x) + U_TRANS


def weight_standardize_stats(w: torch.Tensor, eps: float) -> dict:
    """Row statistics of w [cout, fan_in] in fp64 with the fp32 errors of the way weight_standardize_kernel and
    weight_standardize_bwd_kernel form them (n = fan_in, sums in any order over 256 threads):

      * mean = (sum w) / n: n additions and a division, |d_mean| <= gamma(n + 1) mean|w|;
      * c_i = w_i - mean, one subtraction of the perturbed mean: d_c = d_mean + u32 (|c| + d_mean).  This is the CANCELLATION
        term: for a row 8 + small it is gamma(n) * 8 however small the spread is;
      * var = (sum c_i^2) / n (two-pass): the squares of perturbed c_i move by 2 |c| d_c + d_c^2 each, then one rounding per
        square, n additions, a division: d_var = gamma(n + 4) (var + t) + t, t = mean(2 |c| d_c + d_c^2);
      * r = rsqrtf(var + eps): one rounding of the sum, then _rsqrt_rel."""
    w64 = f64(w)
    n = w64.shape[1]
    eps = f32_const(eps)
    mean = w64.mean(1, keepdim=True)
    c = w64 - mean
    var = (c * c).mean(1, keepdim=True)
    d_mean = gamma(n + 1) * w64.abs().mean(1, keepdim=True)
    d_c = d_mean + U_F32 * (c.abs() + d_mean)
    t = (2.0 * c.abs() * d_c + d_c * d_c).mean(1, keepdim=True)
    d_var = gamma(n + 4) * (var + t) + t
    ve = var + eps
    rel_r = _rsqrt_rel(d_var + U_F32 * ve, ve)
    return dict(w=w64, n=n, mean=mean, c=c, var=var, r=ve.rsqrt(), d_c=d_c, rel_r=rel_r)


def weight_standardize_reference(w: torch.Tensor, gain: torch.Tensor, scale: float, eps: float, to_khwc: bool = False):
    """timm ScaledStdConv2d's weight transform as mg_weight_standardize_bf16 states it, w [cout, cin, kh, kw] bf16, gain [cout]
    bf16 -> (ref, bound) [cout, fan_in] in the column order of the output ((cin, ky, kx), or (ky, kx, cin) with to_khwc):

        out = bf16( (w - mean) * g ),   g = gain * scale * rsqrt(var + eps),  biased variance over the fan-in.

    Statistics: weight_standardize_stats.  g takes two more products (rel_g = rel_r + 2 u32), the element one: its fp32 error is
    |g| d_c + |c g| (rel_g + u32), the first term being the cancellation in w - mean (all that is left for a constant row, whose
    reference is 0), and ``rounded`` adds the bf16 store."""
    cout, cin, kh, kw = w.shape
    T = weight_standardize_stats(w.reshape(cout, -1), eps)
    g = f64(gain).reshape(cout, 1) * f32_const(scale) * T["r"]
    rel_g = T["rel_r"] + 2.0 * U_F32
    ref = T["c"] * g
    err = (g.abs() * T["d_c"] + ref.abs() * (rel_g + U_F32)) * (1.0 + rel_g + U_F32)
    if to_khwc:
        ref, err = (t.reshape(cout, cin, kh * kw).transpose(1, 2).reshape(cout, -1) for t in (ref, err))
    return ref, rounded(ref, err, torch.bfloat16)


def weight_standardize_bwd_reference(w: torch.Tensor, gain: torch.Tensor, dwhat: torch.Tensor, scale: float, eps: float,
                                     dmult: float = 1.0, dw0=None, dgain0=None) -> dict:
    """The closed form in the header of weight_standardize_bwd_kernel, in fp64: with n = (w - mean) r, r = rsqrt(var + eps),
    dh = dwhat * dmult and dn = dh * gain * scale

        dgain = scale * sum(dh n),      dw = r (dn - mean(dn) - n mean(dn n))

    w [cout, fan_in] bf16, gain [cout] bf16, dwhat [cout, fan_in] fp32 (the caller slices the padding off)
    -> {"dw": (ref, bound), "dgain": (ref, bound)} for what the kernel ADDED to fp32 buffers that held dw0 / dgain0.

      * n: r d_c + |n| (rel_r + u32)                                            (statistics: weight_standardize_stats)
      * dh, gain * scale and dn are one product each: d_dn = gamma(3) |dn|, dh n for dgain: gamma(2) relative;
      * m1 = mean(dn): gamma(N + 1) mean|dn| + mean(d_dn);   m2 = mean(dn n): gamma(N + 2) mean|dn n| + mean(|dn| d_n + d_dn |n|);
      * the element: d_inner = d_dn + d_m1 + |n| d_m2 + |m2| d_n + gamma(4) (|dn| + |m1| + |n m2|), times r (rel_r, one rounding);
      * dgain: gamma(N + 3) sum|dh n| + sum(|dh| d_n), times scale;
      * ``+=``: one rounding relative to |buffer + value|, charged to |dw0| + |dw| (the caller subtracts dw0 again in fp64)."""
    T = weight_standardize_stats(w, eps)
    N, r = T["n"], T["r"]
    sc = f32_const(scale)
    n = T["c"] * r
    d_n = (r * T["d_c"] + n.abs() * (T["rel_r"] + U_F32)) * (1.0 + T["rel_r"])
    dh = f64(dwhat) * f32_const(dmult)
    gs = f64(gain).reshape(-1, 1) * sc
    dn = dh * gs
    d_dn = gamma(3) * dn.abs()
    m1, m2 = dn.mean(1, keepdim=True), (dn * n).mean(1, keepdim=True)
    d_m1 = gamma(N + 1) * dn.abs().mean(1, keepdim=True) + d_dn.mean(1, keepdim=True)
    d_m2 = gamma(N + 2) * (dn * n).abs().mean(1, keepdim=True) + (dn.abs() * d_n + d_dn * n.abs()).mean(1, keepdim=True)
    inner = dn - m1 - n * m2
    d_inner = d_dn + d_m1 + n.abs() * d_m2 + m2.abs() * d_n + gamma(4) * (dn.abs() + m1.abs() + (n * m2).abs())
    dw = r * inner
    d_dw = (r * d_inner + dw.abs() * (T["rel_r"] + U_F32)) * (1.0 + T["rel_r"])
    dg = sc * (dh * n).sum(1)
    d_dg = sc * (gamma(N + 3) * (dh * n).abs().sum(1) + (dh.abs() * d_n).sum(1)) + U_F32 * dg.abs()
    if dw0 is not None:
        d_dw = d_dw + U_F32 * (f64(dw0).abs() + dw.abs())
    if dgain0 is not None:
        d_dg = d_dg + U_F32 * (f64(dgain0).abs() + dg.abs())
    return {"dw": (dw, rounded(dw, d_dw, torch.float32)), "dgain": (dg, rounded(dg, d_dg, torch.float32))}


def relu_mean_rows_reference(x: torch.Tensor):
    """x [B, HW, C] bf16 -> (ref, bound) [B, C] of bf16( (sum_p relu(x_p)) / HW ): an fp32 sum of HW non-negative terms in any
    order (the kernel's 32 partial sums and their reduction add zeros exactly) and a division: gamma(HW + 1) of the sum, which
    is its own magnitude sum; one rounding to bf16."""
    HW = x.shape[1]
    ref = torch.relu(f64(x)).mean(1)
    return ref, rounded(ref, gamma(HW + 1) * ref, torch.bfloat16)


def relu_mean_rows_bwd_reference(x: torch.Tensor, g: torch.Tensor):
    """x [B, HW, C], g [B, C] bf16 -> (ref, bound) [B, HW, C] of dx = x > 0 ? bf16( g * (1 / HW) ) : 0.  The gate is exact and is
    the caller's to assert (the bound at a closed gate is FLOOR); an open gate passes g through a rounded reciprocal and a
    rounded product: gamma(2) |g / HW|."""
    HW = x.shape[1]
    ref = torch.where(f64(x) > 0, f64(g)[:, None, :] / HW, torch.zeros((), dtype=torch.float64, device=x.device))
    return ref, map_bound(ref, ref.abs(), 2, torch.bfloat16)


def maxpool3x3s2_bwd_reference(x: torch.Tensor, dy: torch.Tensor):
    """Backward of F.max_pool2d(x, 3, 2, 1), x [B, C, H, W], dy [B, C, Ho, Wo] (bf16 values) -> (ref, bound, count): the window
    maxima are the indices max_pool2d itself returns on the fp32 copy of x (what autograd scatters through: the first maximum
    of a row-major scan, a NaN in place of any maximum, the first valid entry of a window of -inf); the up to four window
    gradients that meet in one element are added in fp64.  The kernel adds them in fp32 and rounds to bf16: gamma(4) sum|dy|.
    count = how many windows feed the element; where it is 1 the kernel's output must be dy's bits."""
    import torch.nn.functional as F
    B, C, H, W = x.shape
    _, idx = F.max_pool2d(x.detach().float().cpu(), 3, stride=2, padding=1, return_indices=True)
    idx = idx.reshape(B, C, -1)
    d = f64(dy).cpu().reshape(B, C, -1)
    ref = torch.zeros(B, C, H * W, dtype=torch.float64).scatter_add_(2, idx, d)
    mag = torch.zeros(B, C, H * W, dtype=torch.float64).scatter_add_(2, idx, d.abs())
    cnt = torch.zeros(B, C, H * W, dtype=torch.float64).scatter_add_(2, idx, torch.ones_like(d))
    ref, mag, cnt = (t.reshape(B, C, H, W) for t in (ref, mag, cnt))
    return ref, rounded(ref, gamma(4) * mag, torch.bfloat16), cnt.to(torch.int64)


WS_ROW_KINDS = ("normal", "large mean", "constant")


def standardize_rows(kind: str, cout: int, cin: int, k: int, seed: int):
    """(w [cout, cin, k, k], gain [cout]) bf16 for the weight-standardisation tests.
      normal      N(0.5, 1): the mean subtraction is visible;
      large mean  8 + 0.01 N(0, 1): in bf16 (spacing 2^-4 above 8, 2^-5 below) most entries ARE 8 and a few sit one step away:
                  mean >> spread, the output is what survives the cancellation in w - mean;
      constant    rows of one repeated value (var = 0, a zero-initialised conv is one); the last row, and row 0, all zero."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(cout, cin, k, k, generator=g)
    if kind == "normal":
        w = z + 0.5
    elif kind == "large mean":
        w = 8.0 + 0.01 * z
    elif kind == "constant":
        w = (torch.randn(cout, 1, 1, 1, generator=g) * 0.3).expand(cout, cin, k, k).clone()
        w[0] = 0.0
        w[-1] = 0.0
    else:
        raise ValueError(kind)
    gain = 1.0 + 0.2 * torch.randn(cout, generator=g)
    return w.to(torch.bfloat16).contiguous(), gain.to(torch.bfloat16)


def relu_rows_input(B: int, HW: int, C: int, seed: int):
    """x [B, HW, C] bf16 with +0, -0 and the smallest positive bf16 (2^-133, a subnormal) among normal values -- an eighth of
    the elements each -- and g [B, C] bf16: the gate of relu_mean_rows_bwd is x > 0, which the first two close and the third opens."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, HW, C, generator=gen).to(torch.bfloat16)
    pick = torch.randint(0, 8, (B, HW, C), generator=gen)
    x[pick == 0] = 0.0
    x[pick == 1] = -0.0
    x[pick == 2] = 2.0 ** -133
    return x, torch.randn(B, C, generator=gen).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------------
# the 3x3 convolutions of the CLIP trunk: forward, input gradient (dgrad), weight gradient (wgrad)
# ---------------------------------------------------------------------------------------------------------------------------
# (B, H, W, Cin, Cout): the smallest shapes that reach each mechanism of the implicit-im2col loader of gemm128_kernel and of
# im2col_t_kernel (cpt = Cin / 8 16-byte chunks per tap, 8 chunks per K-tile, 128-row M-tiles, 64-row tiles of im2col_t)
CONV_SHAPES = [
    (1, 1, 1, 8, 8),             # one pixel: eight of nine taps are padding; cpt = 1: a K-tile spans eight taps
    (2, 1, 5, 24, 16),           # image one pixel high
    (2, 5, 1, 24, 16),           # image one pixel wide
    (3, 5, 7, 40, 24),           # M = 105: a partial M-tile, M % 8 = 1; cpt = 5: taps end inside a K-tile; images end at rows 35, 70
    (2, 9, 15, 72, 40),          # M = 270 = 2 M-tiles + 14 rows, cut inside an image row; batch boundary (135) inside a tile; cpt = 9,
                                 # K = 648: 11 K-tiles, the last one with one chunk
    (1, 12, 12, 192, 136),       # Cin > 64 and a multiple of 64: taps align with K-tiles; two N-tiles, the second with 8 columns
    (2, 12, 12, 768, 768),       # layer 4 of the trunk at batch 2: K = 6912
]
CONV_FAMILIES = ("integers", "gaussian")
EXACT_F32 = 2.0 ** 24            # integers of magnitude <= 2^24 are fp32 values


def conv_shape_id(shape) -> str:
    return "x".join(str(v) for v in shape[:3]) + f",{shape[3]}->{shape[4]}"


def gemm128_splits(M: int, N: int, K: int, split_k: int) -> int:
    """How many split-K slabs gemm_dispatch (csrc/gemm.hip) gives the 128x128 kernel for a bf16 problem that does not go to the
    256x256 kernel (every convolution: its A is not dense), with the default 64 MiB workspace: split_k 1 never splits, n > 1 asks
    for n, 0 asks for min(16, K-tiles / 4, ceil(512 / tiles)) while fewer than 192 tiles exist; the request is clamped to the
    number of K-tiles, each split takes ceil(K-tiles / request) K-tiles and only the splits that start before the end exist."""
    nkt = -(-K // 64)
    tiles = -(-M // 128) * -(-N // 128)
    want = split_k
    if want == 0:
        want = (2 if (tiles < 512 and nkt >= 128) else 1) if tiles >= 192 else min(16, nkt // 4, -(-512 // tiles))
    want = max(1, min(want, nkt))
    assert want * M * -(-N // 128) * 128 * 4 <= 64 << 20, "the default workspace would clamp this request"
    kt_per = -(-nkt // want)
    return -(-nkt // kt_per)


def split_starts_inside_a_tap(K: int, channels: int, splits: int) -> list:
    """The first 16-byte chunk of every split after the first, where it does not fall on a tap boundary (chunk % cpt != 0)."""
    nkt = -(-K // 64)
    kt_per = -(-nkt // splits)
    return [s * kt_per * 8 for s in range(1, splits) if (s * kt_per * 8) % (channels // 8)]


def conv_case(family: str, shape, seed: int = 0, device="cpu") -> dict:
    """Every operand of the three passes of one 3x3 convolution (stride 1, padding 1) with a folded BatchNorm behind it.

      x [B, Cin, H, W] bf16, x_rows [M, Cin] (NHWC rows)      the activation          w [Cout, Cin, 3, 3] bf16   the weight
      g [B, Cout, H, W] bf16, g_rows [M, Cout]                the upstream gradient   scale, bias [Cout] fp32    the folded BatchNorm
      res_out [M, Cout], res_in [M, Cin] bf16                 residuals of the forward / of the dgrad epilogue
      gate_in [M, Cin] bf16                                   the ReLU gate of the dgrad epilogue (open where > 0)
      base [Cout, 9 Cin] fp32                                 what the gradient buffer holds before the wgrad GEMM adds to it

    "integers": values in [-4, 4], scale in {0.5, 1, 2}, gate in {-1, 0, 1}: every product and partial sum of the three passes is
    a multiple of 1/2 below 2^23 (assert_exact_in_fp32 checks it per use), exact in fp32 in ANY order -- MFMA order, split-K
    slabs, an accumulate onto the integer base -- so a kernel's output EQUALS the fp64 reference cast once to the output type.
    "gaussian": the suite's usual operands -- N(0, 1) activations and gradients, weights of scale (9 Cin)^-1/2, scale = |N| + 0.5,
    gates of either sign with +0 / -0 on the corners -- for the per-element bounds."""
    B, H, W, Cin, Cout = shape
    M = B * H * W
    gen = torch.Generator().manual_seed(1000 * seed + 7 * M + Cin + 3 * Cout)
    if family == "integers":
        ints = lambda *s: torch.randint(-4, 5, s, generator=gen).float()
        x, w, g = ints(B, Cin, H, W), ints(Cout, Cin, 3, 3), ints(B, Cout, H, W)
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (Cout,), generator=gen)]
        bias, res_out, res_in, base = ints(Cout), ints(M, Cout), ints(M, Cin), ints(Cout, 9 * Cin)
        gate_in = torch.randint(-1, 2, (M, Cin), generator=gen).float()
    elif family == "gaussian":
        n = lambda *s: torch.randn(*s, generator=gen)
        x, w, g = n(B, Cin, H, W), n(Cout, Cin, 3, 3) * (9 * Cin) ** -0.5, n(B, Cout, H, W)
        scale = n(Cout).abs() + 0.5
        bias, res_out, res_in, base = n(Cout), n(M, Cout), n(M, Cin), n(Cout, 9 * Cin)
        gate_in = n(M, Cin)
        gate_in[0, 0], gate_in[-1, -1] = 0.0, -0.0
    else:
        raise ValueError(family)
    bf = lambda t: t.to(torch.bfloat16).to(device)
    x, w, g = bf(x), bf(w), bf(g)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(M, t.shape[1]).contiguous()
    return dict(family=family, shape=tuple(shape), M=M, x=x, w=w, g=g, x_rows=rows(x), g_rows=rows(g), scale=scale.to(device), bias=bias.to(device),
                res_out=bf(res_out), res_in=bf(res_in), gate_in=bf(gate_in), base=base.to(device))


def conv_weight_rows(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> the forward GEMM operand [Cout, 9 Cin] in (ky, kx, ci) order (conv_weight_relayout mode 0 without its padding)."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def conv_dgrad_weight_rows(w: torch.Tensor, scale: torch.Tensor, flip: bool = True) -> torch.Tensor:
    """The dgrad operand conv_weight_relayout(w, 1, scale) writes, without its padding: [Cin, 9 Cout] bf16,
    W'[ci][(ky, kx), co] = bf16(W[co][ci][2 - ky][2 - kx] * scale[co]) (tests/test_backward_kernels_gpu.py pins it bit for bit).
    flip=False is the seeded fault of the CPU tests."""
    ws = w.float() * scale.float().view(-1, 1, 1, 1)
    if flip:
        ws = ws.flip(2, 3)
    return ws.permute(1, 2, 3, 0).reshape(w.shape[1], -1).to(torch.bfloat16)


def conv2d_dgrad_terms(g: torch.Tensor, w: torch.Tensor = None, scale: torch.Tensor = None, *, wd: torch.Tensor = None):
    """(ref, mag, K) of the input gradient of y = conv2d(x, w * scale[co], padding = 1) as the GEMM it is run as: a 3x3 convolution of
    the upstream gradient g [B, Cout, H, W] with the taps FLIPPED and the channel roles swapped (a transposed convolution),
    rows [B*H*W, Cin] in NHWC order, K = 9 Cout.  Either w [Cout, Cin, 3, 3] and scale [Cout] (the exact w * scale in fp64), or
    wd = the operand the kernel multiplies with, [Cin, >= 9 Cout] in the layout of conv_dgrad_weight_rows (its own bf16
    rounding of w * scale is then the re-layout kernel's business and not charged to the GEMM)."""
    Cout = g.shape[1]
    if wd is None:
        w64 = f64(w) * (1.0 if scale is None else f64(scale).view(-1, 1, 1, 1))
        wt = w64.flip(2, 3).permute(1, 0, 2, 3)                                      # [Cin, Cout, ky, kx]
    else:
        wt = f64(wd)[:, : 9 * Cout].reshape(wd.shape[0], 3, 3, Cout).permute(0, 3, 1, 2)
    return conv2d_terms(g, wt)


def conv2d_wgrad_terms(g_rows: torch.Tensor, x: torch.Tensor):
    """(ref, mag, K) of the weight gradient of y = conv2d(x, w, padding = 1): dW[co][(ci, ky, kx)] = sum over the B*H*W output
    pixels m of g[m][co] * x[pixel m moved by (ky - 1, kx - 1)][ci] (zero outside the image) -- g_rows [B*H*W, Cout] in NHWC order,
    x [B, Cin, H, W]; rows of the result in the weight's own [Cin, 3, 3] flattening, K = B*H*W."""
    M = g_rows.shape[0]
    cols = torch.nn.functional.unfold(f64(x), 3, padding=1).permute(1, 0, 2).reshape(-1, M)        # [Cin 9, M]
    g64 = f64(g_rows)
    return g64.t() @ cols.t(), g64.abs().t() @ cols.abs().t(), M


def im2col_t_reference(x: torch.Tensor) -> torch.Tensor:
    """What mg_im2col_t_bf16 writes for x [B, Cin, H, W] bf16: [9 Cin, round_up(M, 8)], row ci * 9 + ky * 3 + kx, column m = the
    pixel of m moved by (ky - 1, kx - 1) or 0 outside the image; columns [M, round_up(M, 8)) are zero."""
    B, Cin, H, W = x.shape
    M = B * H * W
    out = torch.zeros(9 * Cin, -(-M // 8) * 8, dtype=x.dtype, device=x.device)
    out[:, :M] = torch.nn.functional.unfold(x.float(), 3, padding=1).permute(1, 0, 2).reshape(9 * Cin, M).to(x.dtype)
    return out


def assert_exact_in_fp32(mag: torch.Tensor, lsb: float = 0.5, what: str = "") -> float:
    """The premise of the "integers" family, checked instead of assumed: every partial sum is a multiple of ``lsb`` and at most
    max(mag) in magnitude; such values are fp32 numbers while max(mag) < 2^24 * lsb."""
    top = float(mag.max()) if mag.numel() else 0.0
    assert top < EXACT_F32 * lsb, f"{what}: magnitude sum {top:.6g} is not below 2^24 * {lsb}: fp32 sums are no longer exact"
    return top


def assert_bit_exact(got: torch.Tensor, ref: torch.Tensor, what: str = "") -> None:
    """got == the fp64 reference cast ONCE to got's type, every element (no tolerance; +0 and -0 compare equal)."""
    assert ref.dtype == torch.float64 and got.shape == ref.shape, (got.shape, ref.shape, ref.dtype)
    want = ref.to(got.dtype)
    ok = torch.equal(got, want)
    print(f"[bit-exact] {what}: {'equal' if ok else 'DIFFERENT'}, {got.numel()} elements")
    if not ok:
        bad = (got != want) | torch.isnan(got)
        nz = bad.nonzero()
        lo, hi = nz.min(0).values.tolist(), nz.max(0).values.tolist()
        i = tuple(nz[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ from the exact result; first at {i} (got {float(got[i]):.9g}, "
                             f"exact {float(want[i]):.9g}); bounding box of the offenders " + " x ".join(f"[{a}..{b}]" for a, b in zip(lo, hi)))


def assert_conv_output(family: str, got: torch.Tensor, ref_bound, what: str, mag: torch.Tensor = None) -> None:
    """One output of a convolution pass in its family: "integers" -> assert_bit_exact against ref (and the exactness premise on the
    magnitude sum ``mag``), "gaussian" -> assert_elementwise against (ref, bound)."""
    ref, bound = ref_bound
    if family == "integers":
        assert mag is not None
        assert_exact_in_fp32(mag, 0.5, what)
        assert_bit_exact(got, ref, what)
    else:
        assert_elementwise(got, ref, bound, what)
