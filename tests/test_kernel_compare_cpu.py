"""tests/kernel_compare.py checked on the CPU: no kernel is called, modified or made to misbehave here.

For a GEMM, a causal attention and a LayerNorm an HONEST STAND-IN plays the kernel: the same operation in fp32 with a permuted
summation order, rounded once to the output type (and P rounded to bf16 before PV, as the prefill kernels do).  Faults of the
kinds hand-written kernels have are then written into that result tensor on the host.  Conditions on the helper:

  1. every honest stand-in passes, worst |err| / bound < 1;
  2. every seeded fault fails, and its worst ratio is at least 8 x the bound;
  3. the faults of the table in DESIGN.md ("Test comparators") are ACCEPTED by the whole-tensor criterion
     ||got - ref|| / ||ref|| at the threshold the GPU suite uses for that case.  That is the gap the per-element bound closes;
     the assertion stops anyone from simplifying the helper back to a norm.

Seeds, scales and shapes are those of the GPU tests the cases mirror."""
import math

import pytest
import torch

import epilogue_cases as ec
import kernel_compare as kc

BF16 = torch.bfloat16
FAULT_FACTOR = 8.0


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def old_rel(got, ref):
    """The criterion of the suite before the per-element bound (assert_close / rel_err of tests/test_kernels_gpu.py)."""
    a, b = got.float(), ref.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def check_fault(name, bad, ref, bound, old_tol=None):
    """Condition 2 (and 3 where old_tol is given) for one faulty tensor; returns the figures for the printed table."""
    w = kc.worst_ratio(bad, ref, bound)
    with pytest.raises(AssertionError, match="bounding box"):
        kc.assert_elementwise(bad, ref, bound, name)
    assert w >= FAULT_FACTOR, f"{name}: worst ratio {w:.2f} < {FAULT_FACTOR}"
    old = old_rel(bad, ref)
    print(f"    fault {name:<46s} err/bound {w:9.1f}   rel-L2 {old:.2e}" + (f" < {old_tol} (accepted before)" if old_tol else ""))
    if old_tol is not None:
        assert old < old_tol, f"{name}: the whole-tensor criterion was expected to accept this fault ({old:.3e} >= {old_tol})"
    return w, old


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------------------
def gemm_stand_in(a, w, bias, seed):
    """fp32 accumulation over K in a permuted order (64-wide chunks of a random permutation), bias, one rounding to bf16."""
    K = a.shape[1]
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(seed))
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    af, wf = a.float(), w.float()
    for c in perm.split(64):
        acc += af[:, c] @ wf[:, c].t()
    if bias is not None:
        acc += bias
    return acc.to(BF16)


# (M, N, K, threshold of the mirrored test, faults the old criterion is asserted to accept)
GEMM_CASES = [
    (1216, 512, 4096, 4e-3, {"one element zeroed", "8-wide store dropped at the last tile corner", "8 tail elements x1.5"}),
    (300, 200, 192, 4e-3, {"one element zeroed"}),
    (2048, 4096, 4096, 4e-3, {"8-wide store dropped at the last tile corner"}),
]


@pytest.mark.parametrize("M,N,K,tol,accepted", GEMM_CASES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_gemm_stand_in_and_faults(M, N, K, tol, accepted):
    a = rnd(M, K, seed=1).to(BF16)
    w = rnd(N, K, seed=2, scale=0.05).to(BF16)
    bias = rnd(N, seed=5)
    prod, pmag = kc.product_terms(a, w)
    ref = prod + bias.double()
    bound = kc.gemm_bound(ref, pmag + bias.double().abs(), K, BF16, n_epilogue=1)
    good = gemm_stand_in(a, w, bias, seed=9)
    worst = kc.assert_elementwise(good, ref, bound, f"honest GEMM {M}x{N}x{K}")
    assert worst < 1.0
    assert old_rel(good, ref) < tol
    print(f"  GEMM {M}x{N}x{K}: honest err/bound {worst:.2f}, rel-L2 {old_rel(good, ref):.2e}")

    def tol_of(name):
        return tol if name in accepted else None
    # one element: the one of median magnitude in the last row (a typical element, not a large one)
    j = int(ref[M - 1].abs().argsort()[N // 2])
    bad = good.clone(); bad[M - 1, j] = 0
    check_fault("one element zeroed", bad, ref, bound, tol_of("one element zeroed"))
    bad = good.clone(); bad[M - 1, N - 8:] = 0
    check_fault("8-wide store dropped at the last tile corner", bad, ref, bound, tol_of("8-wide store dropped at the last tile corner"))
    bad = good.clone(); bad[M - 1, N - 8:] = (bad[M - 1, N - 8:].float() * 1.5).to(BF16)
    check_fault("8 tail elements x1.5", bad, ref, bound, tol_of("8 tail elements x1.5"))
    bad = good.clone(); bad[M - 1] = bad[M - 2]
    check_fault("last row equal to the row above", bad, ref, bound)
    bad = good.clone(); bad[M - 16:, N - 16:] = bad[M - 16:, N - 16:].t().clone()
    check_fault("last 16x16 sub-tile transposed", bad, ref, bound)
    # the tail element that misses its bias: the last column whose bias is not small (|bias| > 0.5; N(0,1) entries)
    jb = int((bias.abs() > 0.5).nonzero().max())
    bad = good.clone(); bad[M - 1, jb] = (bad[M - 1, jb].float() - bias[jb]).to(BF16)
    check_fault("tail element without its bias", bad, ref, bound)


def test_gemm_bound_is_tight_not_generous():
    """At K = 192 the honest stand-in comes close to the bound (the output rounding alone reaches u |x| just above a power of
    two): the bound has no slack to hide a fault in.  0.9: some of 60 000 elements lies within 10 % of such a tie."""
    M, N, K = 300, 200, 192
    a = rnd(M, K, seed=1).to(BF16)
    w = rnd(N, K, seed=2, scale=0.05).to(BF16)
    ref, mag = kc.product_terms(a, w)
    bound = kc.gemm_bound(ref, mag, K, BF16)
    worst = kc.worst_ratio(gemm_stand_in(a, w, None, seed=3), ref, bound)
    assert 0.9 < worst < 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------------
# the epilogue contract (kernel_compare.epilogue_reference, epilogue_cases.py)
# ---------------------------------------------------------------------------------------------------------------------------
# 130 x 203 x 128: the shape of the per-element tail path of the GPU matrix (N % 8 = 3, so "the last N % 8 columns" exist)
EPI_SHAPE = (130, 203, 128)
_epi_case = {}


def epi_case():
    if not _epi_case:
        _epi_case["case"] = ec.make_case(*EPI_SHAPE, seed=0)
    return _epi_case["case"]


def test_epilogue_configurations_cover_every_pair():
    """Every pair of 'on' values of {scale, row_scale, bias, act (3), act_n0, aux_mode (4), aux_after, residuals, act_after, C2,
    fp32 output, accumulate} occurs in one configuration at least -- except two activations or two aux modes at once, which no
    descriptor can say -- and each activation / aux mode / residual count also occurs with the other fields OFF (the engine
    entries).  Every entry obeys check_epilogue (cfg asserts accumulate -> fp32)."""
    feats = [ec.features(c) for c in ec.CONFIGS]
    names = sorted(set().union(*feats))
    missing = []
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if a.split("=")[0] == b.split("=")[0] and "=" in a:
                continue
            if not any(a in f and b in f for f in feats):
                missing.append((a, b))
    assert not missing, missing
    assert {c["act"] for c in ec.CONFIGS} == set(kc.ACTS) and {c["aux_mode"] for c in ec.CONFIGS} == set(kc.AUX_MODES)
    assert {c["n_res"] for c in ec.CONFIGS} == {0, 1, 2, 3}
    assert any(c["act"] == "quick_gelu" and c["c2"] for c in ec.CONFIGS) and any(c["aux_mode"] == "quick_gelu_grad" for c in ec.CONFIGS)


def test_epilogue_inputs_hold_the_special_values():
    M, N, _ = EPI_SHAPE
    aux = epi_case()["aux"].float()
    zero = aux == 0
    neg = zero & torch.signbit(aux)
    assert 0.1 < float(zero.float().mean()) < 0.3 and int(neg.sum()) > 1000 and int((zero & ~neg).sum()) > 1000
    rows, cols = ec.corner_index(M, N)
    assert rows == [0, 63, 64, 127, 128, 129] and cols == [0, 7, 8, 202]
    assert bool(zero[rows][:, cols].all())
    (rp, cp), (rn, cn) = ec.big_index(M, N)
    assert float(aux[rp, cp]) == 30.0 and float(aux[rn, cn]) == -30.0
    assert bool((aux > 0).any()) and bool((aux < 0).any())
    # the two GELU derivatives at +-30: exactly 1 and 0 in fp32, and 1 / 0 within the stated error in fp64
    for mode in ("gelu_grad", "quick_gelu_grad"):
        f32 = ec._aux32(torch.tensor([30.0, -30.0]), mode)
        assert float(f32[0]) == 1.0 and abs(float(f32[1])) < 1e-18, (mode, f32)
        f, d_f = kc.aux_factor_terms(torch.tensor([30.0, -30.0]).to(BF16), mode)
        assert abs(float(f[0]) - 1.0) <= float(d_f[0]) + 1e-12 and abs(float(f[1])) <= float(d_f[1]) + 1e-12


@pytest.mark.parametrize("name", [c["name"] for c in ec.CONFIGS])
def test_epilogue_stand_in_passes_every_configuration(name):
    """The honest float32 stand-in of the contract is inside the bound of epilogue_reference for C and for C2, under every
    configuration; where the gate is closed it stores exactly what closed_gate_expectation says."""
    c, case = ec.BY_NAME[name], epi_case()
    R = ec.reference(case, c)
    C, C2 = ec.stand_in(case, c)
    assert kc.assert_elementwise(C, *R["C"], f"stand-in {name} C") < 1.0
    if c["c2"]:
        assert kc.assert_elementwise(C2, *R["C2"], f"stand-in {name} C2") < 1.0
    if c["aux_mode"] == "relu_gate":
        closed = case["aux"] == 0
        assert torch.equal(C[closed], ec.closed_gate_expectation(case, c)[closed])


@pytest.mark.parametrize("fault", ec.FAULTS)
def test_epilogue_seeded_faults_exceed_the_bound(fault):
    """Each slip a hand-written copy of the epilogue can have, written into the stand-in, is at least 8 x outside the bound in
    EVERY configuration it can occur in.  Printed per configuration: the margin.  Faults that only special elements show:
      * "gate with >=" differs where aux is exactly 0.0 or -0.0 and nowhere else (1 / 7 + 1 / 11 of the elements here);
      * "res2 dropped ..." differs in the last N % 8 = 3 columns only;
      * "activation left of act_n0" differs in the columns < act_n0 only, "C2 taken after the activation" in C2 only."""
    case = epi_case()
    M, N, _ = EPI_SHAPE
    hit = 0
    for c in ec.CONFIGS:
        if not ec.fault_applies(fault, c, N):
            continue
        hit += 1
        R = ec.reference(case, c)
        C, C2 = ec.stand_in(case, c, fault)
        which = "C2" if fault == "C2 taken after the activation" else "C"
        bad = C2 if which == "C2" else C
        w, _ = check_fault(f"{fault} [{c['name']}]", bad, *R[which])
        other = C if which == "C2" else C2
        if (which == "C2" or c["c2"]) and fault != "row_scale after the bias":      # the output the fault does not touch stays inside its bound
            assert kc.worst_ratio(other, *R["C" if which == "C2" else "C2"]) < 1.0
        if fault == "gate with >=":
            r = kc.ratios(C, *R["C"])
            assert float(r[case["aux"] != 0].max()) < 1.0, "the fault must be invisible where aux != 0"
        if fault == "res2 dropped in the last N % 8 columns":
            assert float(kc.ratios(C, *R["C"])[:, : N - N % 8].max()) < 1.0
    assert hit >= 2, f"{fault}: only {hit} configurations can show it"


def test_epilogue_reference_agrees_with_linear_reference():
    """Where both can state a case, the two constructors give the same reference, and epilogue_reference is never the looser one:
    both count the same roundings, but a rounding of an epilogue step is relative to the VALUE at hand, which epilogue_reference
    carries, where linear_reference charges it to the magnitude sum -- the bounds part where the product cancels, and stay
    within a factor of two (the accumulation term gamma(K) |A| |W|^T and the output rounding are common to both)."""
    case = epi_case()
    a, w = case["a"], case["w"]
    for name, kw in (("bias", dict(bias=case["bias"])),
                     ("scale_bias_relu", dict(scale=case["scale"], bias=case["bias"], act="relu")),
                     ("bias_gelu", dict(bias=case["bias"], act="gelu")),
                     ("bias_gelu_n0", dict(bias=case["bias"], act="gelu", act_n0=ec.act_n0_of(EPI_SHAPE[1]))),
                     ("bias_res3", dict(bias=case["bias"], residuals=case["res"]))):
        lref, lbound = kc.linear_reference(a, w, **kw)
        eref, ebound = ec.reference(case, ec.BY_NAME[name])["C"]
        assert torch.allclose(lref, eref, rtol=1e-14, atol=1e-14), name
        assert float((ebound / lbound).max()) <= 1.0 + 1e-9 and float((ebound / lbound).min()) > 0.5, (name, float((ebound / lbound).min()))


def test_quick_gelu_terms():
    """quick_gelu through through_activation and quick_gelu_grad_terms against float32 evaluations of the kernels' formulas on a
    dense grid (honest: inside the bound), against autograd in fp64 (the references are the derivative they claim to be), and the
    cancellation of 1 - sg at large positive x stays bounded in ABSOLUTE terms."""
    x32 = torch.linspace(-40, 40, 160001)
    x = x32.double()
    ref = kc.quick_gelu64(x)
    err = kc.through_activation(torch.zeros_like(x), "quick_gelu", x, ref)
    got = ec._act32(x32, "quick_gelu").double()
    assert float(((got - ref).abs() / (err + kc.FLOOR)).max()) < 1.0
    gref, gerr = kc.quick_gelu_grad_terms(x32)
    ggot = ec._aux32(x32, "quick_gelu_grad").double()
    assert float(((ggot - gref).abs() / (gerr + kc.FLOOR)).max()) < 1.0
    xa = x.clone().requires_grad_(True)
    (auto,) = torch.autograd.grad(kc.quick_gelu64(xa).sum(), xa)
    assert float((auto - gref).abs().max()) < 1e-12
    assert 1.09 < float(gref.abs().max()) <= kc.QUICK_GELU_LIPSCHITZ
    # where 1 - sg cancels (large positive x) the error stays ABSOLUTE and of the size |t| u32: no relative blow-up
    assert bool((gerr <= (8.0 * (kc.QUICK_GELU_K * x).abs() + 16.0) * kc.U_F32).all()), float(gerr.max())
    assert kc.QUICK_GELU_K == float(torch.tensor(1.702, dtype=torch.float32))
    # a derivative that is 0.1 % off is far outside
    assert float(((gref - 0.999 * ggot).abs() / (gerr + kc.FLOOR))[x32.abs() < 4].max()) > FAULT_FACTOR


# ---------------------------------------------------------------------------------------------------------------------------
# causal attention
# ---------------------------------------------------------------------------------------------------------------------------
def attention_stand_in(q, k, v, seed, drop_diagonal_of_last_row=False):
    """fp32 scores, exp(t - m) in fp32, row sum of the UNROUNDED weights, weights rounded to bf16 before PV, PV accumulated in
    fp32 over 32-key tiles taken in a permuted order, one rounding of the output to bf16: what the prefill kernels do."""
    S = q.shape[-2]
    t = (q.float() @ k.float().transpose(-1, -2)) * 0.0625
    mask = torch.ones(S, S, dtype=torch.bool).tril()
    if drop_diagonal_of_last_row:
        mask = mask.clone(); mask[S - 1, S - 1] = False
    t = t.masked_fill(~mask, float("-inf"))
    p = torch.exp(t - t.max(-1, keepdim=True).values)
    l = p.sum(-1, keepdim=True)
    pb = p.to(BF16).float()
    vf = v.float()
    tiles = list(range(0, S, 32))
    order = torch.randperm(len(tiles), generator=torch.Generator().manual_seed(seed)).tolist()
    acc = torch.zeros_like(q, dtype=torch.float32)
    for i in order:
        s0 = tiles[i]
        acc += pb[..., s0:s0 + 32] @ vf[..., s0:s0 + 32, :]
    return (acc / l).to(BF16)


def causal_terms(q, k, v):
    S = q.shape[-2]
    return kc.attention_terms(q, k, v, torch.ones(S, S, dtype=torch.bool).tril())


def iid_qkv(S, seed0=81):
    return (rnd(1, 1, S, 256, seed=seed0, scale=0.5).to(BF16), rnd(1, 1, S, 256, seed=seed0 + 1, scale=0.5).to(BF16),
            rnd(1, 1, S, 256, seed=seed0 + 2).to(BF16))


def test_attention_iid_inputs():
    """i.i.d. Gaussian q / k / v (what the GPU tests used alone): the whole-tensor criterion accepts a wrong last row, the
    per-element bound does not -- and NEITHER sees a last row without its diagonal key at S = 2048, because a long softmax row
    averages ~S values.  That is why the structured inputs below exist."""
    # S = 1024, test_attention_forward_kernel_variants (threshold 8e-3)
    q, k, v = iid_qkv(1024)
    T = causal_terms(q, k, v)
    ref, bound = T["ref"], kc.attention_bound(T, 1024)
    good = attention_stand_in(q, k, v, seed=4)
    worst = kc.assert_elementwise(good, ref, bound, "honest attention, i.i.d., S=1024")
    assert worst < 1.0 and old_rel(good, ref) < 8e-3
    bad = good.clone(); bad[0, 0, -1] = bad[0, 0, -2]
    check_fault("S=1024 last query row = the row above it", bad, ref, bound, 8e-3)
    bad = good.clone(); bad[0, 0, -1, -8:] = 0
    check_fault("S=1024 8-wide store dropped in the last row", bad, ref, bound, 8e-3)
    # S = 2048, test_flash_attention_properties_s2048 (threshold 1e-2)
    q, k, v = iid_qkv(2048)
    T = causal_terms(q, k, v)
    ref, bound = T["ref"], kc.attention_bound(T, 2048)
    good = attention_stand_in(q, k, v, seed=5)
    assert kc.assert_elementwise(good, ref, bound, "honest attention, i.i.d., S=2048") < 1.0
    bad = good.clone(); bad[0, 0, -1] = bad[0, 0, -2]
    w = kc.worst_ratio(bad, ref, bound)
    assert w > 1.0 and old_rel(bad, ref) < 1e-2, (w, old_rel(bad, ref))
    print(f"    fault S=2048 i.i.d. last row = the row above: err/bound {w:.1f}, rel-L2 {old_rel(bad, ref):.2e} < 1e-2 (accepted before)")
    nodiag = attention_stand_in(q, k, v, seed=5, drop_diagonal_of_last_row=True)
    w = kc.worst_ratio(nodiag, ref, bound)
    print(f"    fault S=2048 i.i.d. last row without its diagonal key: err/bound {w:.2f}, rel-L2 {old_rel(nodiag, ref):.2e}: "
          f"invisible to any comparator with these inputs")
    assert old_rel(nodiag, ref) < 1e-2


@pytest.mark.parametrize("c", [1.0, 2.0, "tile edges"])
@pytest.mark.parametrize("S", [57, 300, 1024, 2048])
def test_attention_self_dominant_inputs(S, c):
    """k_i = bf16(c q_i + 0.25 noise): each query's own key dominates its row; or ("tile edges", kernel_compare.dominant_edge_keys)
    i.i.d. keys whose tile-edge positions and last key -- the end of a partial tile at S = 57 / 300 -- are 4 q.  The honest
    stand-in stays inside the bound and both causal-boundary faults of the last row are far outside it, at full (1024, 2048)
    and partial (57, 300) last tiles."""
    if c == "tile edges":
        q, k, v = iid_qkv(S, seed0=94)
        k = kc.dominant_edge_keys(q, k)
    else:
        q, k, v = kc.self_dominant_qkv((1, 1, S, 256), c, seed=91)
    T = causal_terms(q, k, v)
    ref, bound = T["ref"], kc.attention_bound(T, S)
    good = attention_stand_in(q, k, v, seed=6)
    worst = kc.assert_elementwise(good, ref, bound, f"honest attention, self-dominant c={c}, S={S}")
    assert worst < 1.0
    nodiag = attention_stand_in(q, k, v, seed=6, drop_diagonal_of_last_row=True)
    # at S = 2048, c = 1 the whole-tensor criterion of test_flash_attention_properties_s2048 still accepts the missing diagonal
    check_fault(f"S={S} c={c} last row without its diagonal key", nodiag, ref, bound, 1e-2 if (S == 2048 and c == 1.0) else None)
    bad = good.clone(); bad[0, 0, -1] = bad[0, 0, -2]
    check_fault(f"S={S} c={c} last query row = the row above it", bad, ref, bound)
    bad = good.clone(); bad[0, 0, -1, -8:] = 0
    check_fault(f"S={S} c={c} 8-wide store dropped in the last row", bad, ref, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# causal attention on the fp8 MFMA (csrc/attention_fwd32_fp8.hip)
# ---------------------------------------------------------------------------------------------------------------------------
F8 = torch.float8_e4m3fn
FP8_FAULT_FACTOR = 10.0
FP8_FAULTS = ("limit -1", "limit +1", "V scale of the neighbouring block", "two keys swapped", "missing rescale")


def pow2_scale(amax):
    """The producer's rule: the smallest power of two 2^e with amax / 2^e <= 448 (1 for an all-zero block)."""
    e = torch.ceil(torch.log2(amax.clamp_min(1e-30) / 448.0))
    return torch.where(amax > 0, torch.exp2(e), torch.ones_like(amax))


class Fp8StandIn:
    """mg_rotary_split_fp8's operands (without the rotary) and mg_attn_prefill_fp8's arithmetic in torch, one head: q / k e4m3 with
    one power-of-two scale per token, V e4m3 with one per (d, 32 keys), keys padded to whole 64-key tiles the way the kernel sees
    them (K rows beyond S: the bytes of row S - 1 with a unit scale; V: zero bytes, unit scales); fp32 scores; the deferred maximum
    with threshold ``defer`` (log2 units: 4 as in the kernel, 0 = the plain running maximum); P = e4m3(16 p) / 16, row sum of the
    unrounded p; O accumulated in fp32 tile by tile; one rounding to bf16.  The MFMA's in-group truncation is not imitated."""

    def __init__(self, q, k, v):
        S = q.shape[0]
        self.S, self.Sp = S, -(-S // 64) * 64
        qf, kf, vf = q.float(), k.float(), v.float()
        sq, sk = pow2_scale(qf.abs().amax(-1, keepdim=True)), pow2_scale(kf.abs().amax(-1, keepdim=True))
        self.qd = (qf / sq).to(F8).float() * sq
        kb = (kf / sk).to(F8).float()
        self.kd = kb * sk
        self.k_all = torch.cat([self.kd, kb[S - 1:S].expand(self.Sp - S, -1)])            # what the kernel multiplies, padding included
        vp = torch.cat([vf, torch.zeros(self.Sp - S, 256)]).view(self.Sp // 32, 32, 256)
        self.sv = pow2_scale(vp.abs().amax(1))                                               # [blocks, 256]
        self.vb = (vp / self.sv[:, None, :]).to(F8).float()                                  # [blocks, 32, 256] e4m3 values
        self.vd = (self.vb * self.sv[:, None, :]).view(self.Sp, 256)[:S]

    def run(self, defer=4.0, rows=None, fault=None):
        """out bf16 [len(rows), 256], lse fp32 [len(rows)] of the query rows ``rows`` (default: all), ``fault`` seeded into them."""
        S, Sp = self.S, self.Sp
        rows = torch.arange(S) if rows is None else torch.as_tensor(rows)
        lim = rows.clone()
        if fault == "limit -1":
            lim -= 1
        elif fault == "limit +1":
            lim += 1
        t2 = (self.qd[rows] @ self.k_all.t()) * (0.0625 * 1.4426950408889634)               # fp32, log2 units
        n = len(rows)
        m2 = torch.full((n,), -1e30)
        lsum, O = torch.zeros(n), torch.zeros(n, 256)
        for kv0 in range(0, Sp, 64):
            act = lim >= kv0                                                                 # rows that see a key of this tile
            if not bool(act.any()):
                break
            vis = torch.arange(kv0, kv0 + 64)[None, :] <= lim[:, None]
            sn = t2[:, kv0:kv0 + 64].masked_fill(~vis, -1e30)
            cand = sn.amax(-1)
            mnew = torch.where(cand > m2 + defer, cand, m2)
            alpha = torch.exp2(m2 - mnew)
            m2 = mnew
            p = torch.exp2(sn - m2[:, None])
            lsum = lsum * alpha + p.sum(-1)
            if fault != "missing rescale":
                O = O * alpha[:, None]
            p8 = (p * 16.0).to(F8).float() * 0.0625
            for b in range(2):
                blk = kv0 // 32 + b
                vb, sv = self.vb[blk], self.sv[blk]
                c = (p8[:, 32 * b:32 * b + 32] @ vb) * sv
                own = (rows // 32 == blk)                                                    # the block of the row's own (newest) key
                if fault == "V scale of the neighbouring block" and bool(own.any()):
                    c[own] = (p8[own, 32 * b:32 * b + 32] @ vb) * self.sv[blk ^ 1]
                if fault == "two keys swapped" and bool(own.any()):                          # keys r and r ^ 1 exchange their V bytes
                    for i in own.nonzero().flatten().tolist():
                        r = int(rows[i]) % 32
                        vs = vb.clone()
                        vs[[r, r ^ 1]] = vb[[r ^ 1, r]]
                        c[i] = (p8[i, 32 * b:32 * b + 32] @ vs) * sv
                O = O + c
        return (O / lsum[:, None]).to(BF16), (m2 + torch.log2(lsum)) * 0.6931471805599453


def fp8_fault_rows(S):
    """Single tile-edge rows: the last r < S - 1 with r % 64 == 63, the last with r % 64 == 0, the last row (of a partial 128-block
    unless S % 128 == 0), the row before it."""
    return {"r % 64 == 63": ((S - 1) // 64) * 64 - 1, "r % 64 == 0": ((S - 1) // 64) * 64, "last": S - 1, "last - 1": S - 2}


_FP8_CASES = {}


def fp8_case(kind, S):
    if (kind, S) not in _FP8_CASES:
        q, k, v = kc.fp8_attention_inputs(kind, (S, 256), seed=91)
        st = Fp8StandIn(q, k, v)
        T = kc.fp8_attention_terms(st.qd, st.kd, st.vd, torch.ones(S, S, dtype=torch.bool).tril())
        _FP8_CASES[(kind, S)] = (st, T, kc.fp8_attention_bound(T, S), kc.fp8_lse_bound(T, S))
    return _FP8_CASES[(kind, S)]


@pytest.mark.parametrize("S", [193, 300, 1024])
@pytest.mark.parametrize("kind", kc.FP8_ATTN_INPUTS + ("i.i.d.",))
def test_fp8_attention_stand_in_is_inside_the_bound(kind, S):
    """The honest stand-in, with the kernel's deferral threshold and with the plain running maximum, stays inside
    fp8_attention_bound / fp8_lse_bound for every input kind (and for i.i.d. inputs of the GPU test's scale)."""
    if kind == "i.i.d.":
        st = Fp8StandIn(rnd(S, 256, seed=91, scale=0.7).to(BF16), rnd(S, 256, seed=92, scale=0.7).to(BF16), rnd(S, 256, seed=93, scale=0.7).to(BF16))
        T = kc.fp8_attention_terms(st.qd, st.kd, st.vd, torch.ones(S, S, dtype=torch.bool).tril())
        bound, lb = kc.fp8_attention_bound(T, S), kc.fp8_lse_bound(T, S)
    else:
        st, T, bound, lb = fp8_case(kind, S)
    for defer in (4.0, 0.0):
        out, lse = st.run(defer=defer)
        assert kc.assert_elementwise(out, T["ref"], bound, f"fp8 stand-in, {kind}, S={S}, deferral {defer}") < 1.0
        kc.assert_elementwise(lse, T["lse"], lb, f"fp8 stand-in lse, {kind}, S={S}, deferral {defer}")


@pytest.mark.parametrize("S", [193, 300, 1024])
def test_fp8_attention_seeded_faults_exceed_the_bound(S):
    """Each fault, seeded into ONE tile-edge row, leaves fp8_attention_bound by at least 10 x on at least one input kind (the
    table names it, with the whole-tensor rel-L2 of the output that holds the faulty row: the GPU test's criterion is < 3e-2)."""
    print()
    for where, r in fp8_fault_rows(S).items():
        for fault in FP8_FAULTS:
            if fault == "limit +1" and r == S - 1 and S % 64 == 0:
                continue        # key S would open a tile of its own, which the tile loop (ceil(S / 64) tiles) never reaches: no such fault
            best, best_kind, line = 0.0, None, []
            for kind in kc.FP8_ATTN_INPUTS:
                st, T, bound, _ = fp8_case(kind, S)
                good, _ = st.run()
                bad_row, _ = st.run(rows=[r], fault=fault)
                w = kc.worst_ratio(bad_row, T["ref"][r:r + 1], bound[r:r + 1])
                bad = good.clone(); bad[r] = bad_row[0]
                line.append(f"{kind} {w:.3g} (rel-L2 {old_rel(bad, T['ref']):.3f})")
                if w > best:
                    best, best_kind = w, kind
            print(f"    S={S} row {r} ({where}) {fault:<36s} caught by {best_kind!r} at {best:.3g} x the bound   [" + ", ".join(line) + "]")
            assert best >= FP8_FAULT_FACTOR, f"S={S} row {r} ({where}): {fault}: no input kind reaches {FP8_FAULT_FACTOR} x the bound (best {best:.3g}, {best_kind})"


# ---------------------------------------------------------------------------------------------------------------------------
# causal attention, backward
# ---------------------------------------------------------------------------------------------------------------------------
def attention_backward_stand_in(q, k, v, dO_rows, out_rows, lse):
    """What the backward kernels do, in fp32: P from the saved lse, rounded to bf16 for dV and dS; D from the saved bf16 O;
    dS rounded to bf16 before dQ / dK; one rounding of each output to bf16."""
    return {name: g.to(BF16) for name, g in attention_backward_stand_in32(q, k, v, dO_rows, out_rows, lse).items()}


def attention_backward_stand_in32(q, k, v, dO_rows, out_rows, lse):
    """attention_backward_stand_in before the output rounding: the fp32 accumulators an epilogue is handed."""
    B, H, S, D = q.shape
    dO = dO_rows.float().reshape(B, S, H, D).permute(0, 2, 1, 3)
    O = out_rows.float().reshape(B, S, H, D).permute(0, 2, 1, 3)
    t = (q.float() @ k.float().transpose(-1, -2)) * 0.0625
    t = t.masked_fill(~torch.ones(S, S, dtype=torch.bool).tril(), float("-inf"))
    pb = torch.exp(t - lse[..., None]).to(BF16).float()
    dV = pb.transpose(-1, -2) @ dO
    dS = (pb * (dO @ v.float().transpose(-1, -2) - (dO * O).sum(-1, keepdim=True))).to(BF16).float()
    return {"dq": dS @ k.float() * 0.0625, "dk": dS.transpose(-1, -2) @ q.float() * 0.0625, "dv": dV}


@pytest.mark.parametrize("inputs", ["i.i.d.", "self c=1"])
@pytest.mark.parametrize("S", [300, 1024])
def test_attention_backward_stand_in_and_faults(S, inputs):
    """dQ / dK / dV against kernel_compare.attention_backward_reference, which takes O and lse as the backward kernel reads them
    (the forward stand-in's bf16 O, an fp32 lse): the honest stand-in is below 1, and a dropped 8-wide store or a row copied from
    the row above -- in the last row and in a middle row of each gradient -- is at least 8 x the bound.  (With D taken from the
    exact softmax instead, sum_d |dO| bound(O) enters every element of dQ / dK and the same drops reach 0.9 .. 3.8 only.)
    The tile-edge inputs are left out here: a row whose softmax is one-hot has dQ = 0 exactly, so a dropped store is no fault."""
    if inputs == "i.i.d.":
        q, k, v = iid_qkv(S, seed0=20)
    else:
        q, k, v = kc.self_dominant_qkv((1, 1, S, 256), 1.0, seed=27)
    dO = rnd(S, 256, seed=23).to(BF16)
    out = kc.rows_of(attention_stand_in(q, k, v, seed=4))
    lse = causal_terms(q, k, v)["lse"].float()
    R = kc.attention_backward_reference(q, k, v, dO, out, lse)
    good = attention_backward_stand_in(q, k, v, dO, out, lse)
    for name in ("dq", "dk", "dv"):
        ref, bound = R[name]
        assert kc.assert_elementwise(good[name], ref, bound, f"honest attention backward {name}, {inputs}, S={S}") < 1.0
        for row in (S - 1, S // 2):
            bad = good[name].clone(); bad[0, 0, row, -8:] = 0
            check_fault(f"S={S} {inputs} {name}: 8-wide store dropped in row {row}", bad, ref, bound)
            bad = good[name].clone(); bad[0, 0, row] = bad[0, 0, row - 1]
            check_fault(f"S={S} {inputs} {name}: row {row} = the row above it", bad, ref, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# causal attention, backward: the MERGED output dqkv = [dq | dk | dv] with the inverse rotary in the epilogue
# ---------------------------------------------------------------------------------------------------------------------------
MERGED_OLD_TOL = 6e-3       # the GPU suite's norm against attn_bwd + rotary_merge_bwd (test_attention_backward_kernel_variants)


def rotary_tables32(rows, rot_dim):
    """The fp32 GPT-J tables [rows, rot_dim / 2] as the GPU tests build them."""
    inv = 1.0 / (10000 ** (torch.arange(0, rot_dim, 2, dtype=torch.float32) / rot_dim))
    ang = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None, :]
    return ang.sin().contiguous(), ang.cos().contiguous()


def merged_epilogue_row(x, sin_row, cos_row, rot_dim, fault=None, group=0):
    """One row of a dq / dk head through the merged epilogue: x fp32 [256] (an accumulator row, already scaled), the inverse turn
    in fp32 -- two rounded products, one addition -- with ONE table row, one rounding to bf16.  fault, in the 4-column group
    ``group`` (the 4 consecutive columns = 2 pairs one lane turns): "sin sign" -- the sine negated; "pair partner" -- the
    partner element taken from the group's other pair."""
    xe, xo = x[0:rot_dim:2].clone(), x[1:rot_dim:2].clone()
    s, c = sin_row.clone(), cos_row
    pe, po = xo.clone(), xe.clone()                      # the partner of the even / of the odd element of a pair
    i = 2 * group
    if fault == "sin sign":
        s[i:i + 2] = -s[i:i + 2]
    elif fault == "pair partner":
        pe[i], pe[i + 1], po[i], po[i + 1] = xo[i + 1], xo[i], xe[i + 1], xe[i]
    else:
        assert fault is None, fault
    y = x.clone()
    y[0:rot_dim:2] = xe * c + pe * s
    y[1:rot_dim:2] = xo * c - po * s
    return y.to(BF16)


def merged_stand_in(g32, sin_t, cos_t, rot_dim):
    """The merged output [B*S, 3 H 256] from the fp32 accumulators {dq, dk, dv} [B, H, S, 256] (attention_backward_stand_in32): dq and
    dk turned back by the table row of their own position in fp32, everything rounded once, rows placed as grad_row_ptr states."""
    S = g32["dq"].shape[2]
    cols = []
    for name in ("dq", "dk", "dv"):
        x = g32[name].clone()
        if name != "dv" and rot_dim:
            s, c = sin_t[:S], cos_t[:S]
            xe, xo = x[..., 0:rot_dim:2].clone(), x[..., 1:rot_dim:2].clone()
            x[..., 0:rot_dim:2] = xe * c + xo * s
            x[..., 1:rot_dim:2] = xo * c - xe * s
        cols.append(kc.rows_of(x.to(BF16)))
    return torch.cat(cols, 1)


def merged_old_criterion(got, two_pass, d):
    """What the GPU suite asked of the merged tensor before the per-element bound: the dv section bit for bit, rel-L2 of the dq
    and of the dk section against the two-pass form -> (dv equal, the larger of the two norms)."""
    return (torch.equal(got[:, 2 * d:], two_pass[:, 2 * d:]),
            max(old_rel(got[:, sl], two_pass[:, sl]) for sl in (slice(0, d), slice(d, 2 * d))))


@pytest.mark.parametrize("inputs", kc.MERGED_BWD_FAMILIES)
@pytest.mark.parametrize("B,S", [(2, 300), (1, 2048)])
def test_merged_attention_backward_stand_in_and_faults(B, S, inputs):
    """dqkv against kernel_compare.merged_backward_reference, H = 2, rot_dim 64, tables [S + 3, 32] as the GPU tests use them.
    The honest stand-in (attention_backward_stand_in32 + the inverse rotary in fp32 + one rounding) is inside the bound.  Each
    fault an epilogue can have -- the table row of the position before / after, the sine's sign in one 4-column group, a pair
    partner from the neighbouring pair, a dropped 8-wide store, the row in the neighbouring batch item's slot, a dq head in the
    dk section -- seeded into ONE row (the last row of a 32-row tile in mid-sequence, and the last row of the sequence) of the
    last batch item's last head, is at least 8 x the bound.  With the i.i.d. inputs (the kind the GPU tests of this tensor use)
    the position, sign and dropped-store faults PASS what the suite asked of it before (merged_old_criterion against the two-pass
    form, < 6e-3): the hole the per-element bound closes.  With the self-dominant inputs most dq rows are nearly zero (a one-hot
    softmax row has dS = 0), one row is a large share of the section's norm and the norm sees some of these faults too: its
    figure is printed, not asserted."""
    H, rot = 2, 64
    d = H * 256
    iid = inputs == "i.i.d."
    q, k, v, dO = kc.merged_backward_inputs(inputs, B, H, S)
    sin_t, cos_t = rotary_tables32(S + 3, rot)
    out = kc.rows_of(attention_stand_in(q, k, v, seed=4))
    lse = causal_terms(q, k, v)["lse"].float()
    R = kc.attention_backward_reference(q, k, v, dO, out, lse)
    ref, bound = kc.merged_backward_reference(R, sin_t, cos_t, rot, B, H, S)
    g32 = attention_backward_stand_in32(q, k, v, dO, out, lse)
    del R
    good = merged_stand_in(g32, sin_t, cos_t, rot)
    two_pass = merged_stand_in({n: g.to(BF16).float() for n, g in g32.items()}, sin_t, cos_t, rot)
    clean = kc.assert_elementwise(good, ref, bound, f"honest merged attention backward, {inputs}, B={B} S={S}")
    assert clean <= 1.0
    dv_same, clean_old = merged_old_criterion(good, two_pass, d)
    print(f"    clean: err/bound {clean:.3f}, rel-L2 against the two-pass form {clean_old:.2e}")
    assert dv_same and clean_old < MERGED_OLD_TOL
    b, h = B - 1, H - 1
    sect = {"dq": 0, "dk": 1, "dv": 2}
    col = lambda name, h_=h: sect[name] * d + h_ * 256

    def seeded(fault, bad, hole):
        w, _ = check_fault(f"B={B} S={S} {inputs}: {fault}", bad, ref, bound)
        if hole:
            same, old = merged_old_criterion(bad, two_pass, d)
            print(f"{'':>10s}rel-L2 against the two-pass form {old:.2e}" + (f" < {MERGED_OLD_TOL}: accepted before" if iid else ""))
            if iid:
                assert same and old < MERGED_OLD_TOL, f"{fault}: the old criterion was expected to accept this ({old:.3e})"

    for s in (32 * (S // 64) + 31, S - 1):
        r = b * S + s
        for name in ("dq", "dk"):
            x, c0 = g32[name][b, h, s], col(name)
            for step in (1, -1):
                bad = good.clone(); bad[r, c0:c0 + 256] = merged_epilogue_row(x, sin_t[s + step], cos_t[s + step], rot)
                seeded(f"{name} row {s} turned by the angles of position {s + step}", bad, True)
            bad = good.clone(); bad[r, c0:c0 + 256] = merged_epilogue_row(x, sin_t[s], cos_t[s], rot, "sin sign")
            seeded(f"{name} row {s}: sine negated in columns 0..3", bad, True)
            # swapped partners: in the 4-column group where that moves this row most (a kernel with this fault has it in every row
            # and group; two pairs that happen to hold similar values in this one row would say nothing about the comparator)
            rows = [merged_epilogue_row(x, sin_t[s], cos_t[s], rot, "pair partner", g) for g in range(rot // 4)]
            g = max(range(rot // 4), key=lambda g: float((rows[g].float() - good[r, c0:c0 + 256].float()).abs().max()))
            bad = good.clone(); bad[r, c0:c0 + 256] = rows[g]
            seeded(f"{name} row {s}: pair partners swapped in columns {4 * g}..{4 * g + 3}", bad, False)
            for c8 in (0, 248):
                bad = good.clone(); bad[r, c0 + c8:c0 + c8 + 8] = 0
                seeded(f"{name} row {s}: 8-wide store at column {c8} dropped", bad, True)
        bad = good.clone(); bad[r, col("dv") + 248:col("dv") + 256] = 0
        seeded(f"dv row {s}: 8-wide store at column 248 dropped", bad, False)
        bad = good.clone(); bad[r, col("dk"):col("dk") + 256] = good[r, col("dq"):col("dq") + 256]
        seeded(f"row {s}: the dq head stored in the dk section", bad, False)
        if B > 1:
            for name in ("dq", "dk", "dv"):
                bad = good.clone(); bad[(b - 1) * S + s, col(name):col(name) + 256] = good[r, col(name):col(name) + 256]
                seeded(f"{name} row {s} written to the neighbouring batch item", bad, False)


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,d", [(37, 512), (8, 4096)])
def test_layernorm_stand_in_and_faults(rows, d):
    x = (rnd(rows, d, seed=41) * 2 + 0.3).to(BF16)
    g = rnd(d, seed=42) * 0.1 + 1
    b = rnd(d, seed=43) * 0.1
    T = kc.layernorm_terms(x, g, b, 1e-5)
    ref, bound = T["ref"], kc.layernorm_bound(T, d)
    perm = torch.randperm(d, generator=torch.Generator().manual_seed(7))
    xf = x.float()
    mean = xf[:, perm].sum(-1, keepdim=True) / d
    var = ((xf - mean)[:, perm] ** 2).sum(-1, keepdim=True) / d
    good = ((xf - mean) * torch.rsqrt(var + 1e-5) * g + b).to(BF16)
    worst = kc.assert_elementwise(good, ref, bound, f"honest LayerNorm {rows}x{d}")
    assert worst < 1.0
    j = int(ref[rows - 1].abs().argsort()[d // 2])
    bad = good.clone(); bad[rows - 1, j] = 0
    check_fault("one element zeroed", bad, ref, bound)
    bad = good.clone(); bad[rows - 1, d - 8:] = 0
    check_fault("8-wide store dropped at the end of the last row", bad, ref, bound)
    bad = good.clone(); bad[rows - 1] = bad[rows - 2]
    check_fault("last row equal to the row above", bad, ref, bound)
    jb = int((b.abs() > 0.05).nonzero().max())
    bad = good.clone(); bad[rows - 1, jb] = (bad[rows - 1, jb].float() - b[jb]).to(BF16)
    check_fault("tail element without its beta", bad, ref, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# the comparator itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_failure_message_locates_the_fault():
    ref = torch.arange(64 * 48, dtype=torch.float64).reshape(64, 48) / 7 + 1
    bound = kc.rounded(ref, torch.zeros_like(ref), BF16)
    got = ref.to(BF16)
    assert kc.assert_elementwise(got, ref, bound, "exact rounding") <= 1.0      # half an ulp just above a power of two = u |x|
    bad = got.clone(); bad[48:64, 40:48] = 0
    with pytest.raises(AssertionError) as e:
        kc.assert_elementwise(bad, ref, bound, "corner")
    m = str(e.value)
    assert "[48..63] x [40..47]" in m and "128 of 3072 elements over" in m and "worst |err|/bound" in m and "at index (" in m
    nan = got.clone(); nan[3, 5] = float("nan")
    with pytest.raises(AssertionError, match=r"\[3\.\.3\] x \[5\.\.5\].*1 not finite"):
        kc.assert_elementwise(nan, ref, bound, "nan")
    with pytest.raises(AssertionError):
        kc.assert_elementwise(got, ref.float(), bound, "fp32 reference refused")


def test_constants():
    assert kc.U_BF16 == 2.0 ** -8 and kc.U_F32 == 2.0 ** -24
    # bf16 rounds to nearest even: 1 + 2^-8 is a tie and goes to 1, the half-ulp error equals u |x| / (1 + u)
    assert float(torch.tensor(1 + 2.0 ** -8).to(BF16)) == 1.0
    assert float(torch.tensor(1 + 3 * 2.0 ** -8).to(BF16)) == 1 + 2.0 ** -6
    assert math.isclose(kc.gamma(4096), 4096 * 2.0 ** -24 / (1 - 4096 * 2.0 ** -24))
    x = torch.linspace(-6, 6, 24001, dtype=torch.float64, requires_grad=True)
    y = 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    (gr,) = torch.autograd.grad(y.sum(), x)
    assert 1.12 < float(gr.abs().max()) <= kc.GELU_LIPSCHITZ


# ---------------------------------------------------------------------------------------------------------------------------
# gradient accumulation: a window of N micro-steps against the sum of its parts
# ---------------------------------------------------------------------------------------------------------------------------
ACC_NOISE = 1e-6          # injected, relative, on top of the re-ordered fp32 sums: the level of the column sums' atomics


def _micro_gradient(src, seed):
    """One micro-step's gradient of a bias-like / weight-like tensor the way a column-sum kernel forms it: the rows of ``src``
    added in fp32 in an order that differs from run to run (32-row chunks of a permutation), with atomic-like noise on top."""
    g = torch.Generator().manual_seed(seed)
    acc = torch.zeros(src.shape[1:], dtype=torch.float32)
    for c in torch.randperm(src.shape[0], generator=g).split(32):
        acc += src[c].sum(0)
    return acc * (1.0 + ACC_NOISE * torch.randn(acc.shape, generator=g))


def _window(srcs, seed, start=None):
    """N parts accumulated into ONE fp32 buffer, ``buf += g_i``, in yet another order."""
    buf = torch.zeros(srcs[0].shape[1:], dtype=torch.float32) if start is None else start.clone()
    for i, s in enumerate(srcs):
        buf += _micro_gradient(s, seed + i)
    return buf


@pytest.mark.parametrize("shape", [(1056,), (64, 136)], ids=["bias", "weight"])
def test_accumulation_stand_in_and_faults(shape):
    """kernel_compare.accumulation_bound on the host: a float32 stand-in of 'three micro-steps into one buffer' passes; the five
    ways a gradient sink or the engine around it can break the window are each far over the bound.  Rows per micro-step differ
    (64 / 128 / 96) as the truncated sequence lengths of the GPU test do."""
    N = 3
    srcs = [rnd(r, *shape, seed=50 + i, scale=0.02) for i, r in enumerate((64, 128, 96))]
    parts = [_micro_gradient(s, 100 + i) for i, s in enumerate(srcs)]
    repeats = [_micro_gradient(s, 200 + i) for i, s in enumerate(srcs)]
    ref, bound, self_ratio, invisible = kc.accumulation_conditions(parts, repeats, f"stand-in {shape}")
    assert self_ratio <= 1.0 and not invisible
    good = _window(srcs, 300)
    out = kc.assert_accumulation(good, parts, repeats, f"honest window {shape}")
    assert out["worst"] < 1.0 and out["zero_parts"] == []
    print(f"  accumulation {shape}: honest err/bound {out['worst']:.3f}, reference against reference {out['self']:.3f}")
    # the five faults, each written the way the engine would commit it
    check_fault("the last part overwrites (only g_N remains)", _micro_gradient(srcs[-1], 302), ref, bound)
    bad = good.clone()
    bad.reshape(-1)[-3:] -= parts[0].reshape(-1)[-3:]
    check_fault("first part missing from the last 3 elements (a cs[:V]-style slice)", bad, ref, bound)
    assert "3 of" in kc.describe_failure(bad, ref, bound)
    check_fault("one part added twice", good + _micro_gradient(srcs[1], 310), ref, bound)
    check_fault("buffer starts from the previous window's contents", _window(srcs, 300, start=_window(srcs, 400)), ref, bound)
    check_fault("result scaled by 1/N (scale applied in backward instead of at the step)", good / N, ref, bound)


def test_accumulation_conditions_refuse_weak_inputs():
    """The two conditions are checked before a window is looked at: a reference noisier than its own bound is reported as such,
    and a part too small to be missed is listed (an identically zero one flagged as excusable, any other not)."""
    srcs = [rnd(64, 256, seed=60 + i, scale=0.02) for i in range(3)]
    parts = [_micro_gradient(s, 100 + i) for i, s in enumerate(srcs)]
    repeats = [_micro_gradient(s, 200 + i) for i, s in enumerate(srcs)]
    # run-to-run noise that the repeat sampled (one element moved by 1e-3 of the largest) is covered by 4 x the sample itself
    rep_b = [p.clone() for p in parts]
    rep_b[1][7] += 1e-3 * parts[1].abs().max()
    _, _, self_ratio, _ = kc.accumulation_conditions(parts, rep_b, "noise seen by the sample")
    assert 0.2 < self_ratio <= 0.25
    # noise in rare discrete jumps is NOT covered: a repeat that happened to agree measures nothing, and a window that jumped fails
    got = _window(srcs, 300)
    got[11] += 7e-5 * parts[2][11]
    quiet = [p.clone() for p in parts]
    with pytest.raises(AssertionError, match="bounding box"):
        kc.assert_accumulation(got, parts, quiet, "one quiet sample")
    faint = [parts[0], parts[1] * 1e-7, parts[2]]
    faint_r = [repeats[0], repeats[1] * 1e-7, repeats[2]]
    _, _, _, invisible = kc.accumulation_conditions(faint, faint_r, "faint part")
    assert [(i, z) for i, _, z in invisible] == [(1, False)]
    with pytest.raises(AssertionError, match="below 100"):
        kc.assert_accumulation(_window(srcs, 300), faint, faint_r, "faint part")
    zero = [parts[0], torch.zeros_like(parts[1]), parts[2]]
    zero_r = [repeats[0], torch.zeros_like(parts[1]), repeats[2]]
    got = parts[0] + parts[2]
    assert kc.assert_accumulation(got, zero, zero_r, "zero part")["zero_parts"] == [1]
    # parts that cancel: the first term follows sum |g_i|, the floor the rms of the (small) sum -- the bound stays far below the parts
    cancel = [parts[0], -parts[0] + 1e-3 * parts[2], parts[2]]
    cancel_r = [repeats[0], -repeats[0] + 1e-3 * repeats[2], repeats[2]]
    ref, bound, self_ratio, _ = kc.accumulation_conditions(cancel, cancel_r, "cancelling parts")
    assert self_ratio <= 1.0 and float((bound / kc.f64(parts[0]).abs().clamp_min(1e-30)).median()) < 1e-4
    # an all-zero tensor is compared, not divided by zero
    z = [torch.zeros(8)] * 3
    assert kc.assert_accumulation(torch.zeros(8), z, z, "all zero")["worst"] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# the NF-ResNet kernels: weight standardisation (forward, backward), ReLU + mean over positions (forward, backward)
# ---------------------------------------------------------------------------------------------------------------------------
WS_SCALE, WS_EPS = 1.7139588594436646, 1e-5        # gamma of ReLU (times fan_in^-1/2 below), ScaledStdConv2d's eps


def check_exceeds(name, bad, ref, bound):
    """A seeded fault whose size is fixed by the shape (1 / (2 fan_in), 1 / HW ...) and need not reach FAULT_FACTOR bounds: it
    must be over the bound, and the figure is printed."""
    w = kc.worst_ratio(bad, ref, bound)
    with pytest.raises(AssertionError, match="bounding box"):
        kc.assert_elementwise(bad, ref, bound, name)
    print(f"    fault {name:<58s} err/bound {w:9.1f}   rel-L2 {old_rel(bad, ref):.2e}")
    return w


def ws_stats32(wf, eps, fault=None, ldo=None):
    """mean, r of weight_standardize_kernel in float32 (sums in a permuted order), with the seeded slips."""
    N = wf.shape[1]
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3))
    mean = wf[:, perm].sum(1, keepdim=True) / (ldo if fault == "mean over ldo" else N)
    var = ((wf - mean)[:, perm] ** 2).sum(1, keepdim=True) / (N - 1 if fault == "unbiased variance" else N)
    r = 1.0 / (var.sqrt() + eps) if fault == "eps outside the root" else torch.rsqrt(var + eps)
    return mean, r


def ws_stand_in(w, gain, scale, eps, to_khwc=False, fault=None, ldo=None):
    cout, cin, kh, kw = w.shape
    wf = w.float().reshape(cout, -1)
    mean, r = ws_stats32(wf, eps, fault, ldo)
    g = gain.float().reshape(cout, 1) * torch.tensor(scale, dtype=torch.float32) * r
    out = (wf - mean) * g
    if to_khwc:
        out = out.reshape(cout, cin, kh * kw).transpose(1, 2).reshape(cout, -1)
    return out.to(BF16)


def ws_bwd_stand_in(w, gain, dwhat, scale, eps, dmult, dw0, dgain0, fault=None, drop=-1):
    """weight_standardize_bwd_kernel in float32: returns what it ADDED to the buffers (the difference formed in fp64)."""
    wf = w.float().reshape(w.shape[0], -1)
    N = wf.shape[1]
    mean, r = ws_stats32(wf, eps, fault)
    sc = torch.tensor(scale, dtype=torch.float32)
    gs = gain.float().reshape(-1, 1) * sc
    n = (wf - mean) * r
    dh = dwhat * torch.tensor(dmult, dtype=torch.float32)
    dn = dh * gs
    m1, m2 = dn.sum(1, keepdim=True) / N, (dn * n).sum(1, keepdim=True) / N
    dw = dw0 + r * (dn - m1 - n * m2)
    dg = dgain0 + sc * (dh * n).sum(1)
    if fault == "one gradient element dropped":
        dw[-1, drop] = dw0[-1, drop]
    return dw.double() - dw0.double(), dg.double() - dgain0.double()


@pytest.mark.parametrize("kind", kc.WS_ROW_KINDS)
@pytest.mark.parametrize("cout,cin,k", [(16, 3, 3), (40, 24, 3), (8, 2048, 1)])
def test_weight_standardize_stand_in_and_faults(cout, cin, k, kind):
    """kernel_compare.weight_standardize_reference / weight_standardize_bwd_reference: the float32 restatement of the two kernels
    is inside the bound for every row kind; the slips are outside it wherever the arithmetic lets them show:
      * forward, bf16 output: a biased / unbiased mix-up is 1 / (2 fan_in) of the value -- above u_bf16 at fan-in 27 only; eps
        outside the root shows where var is not >> eps (the 'large mean' rows); the mean over ldo shows wherever the mean is not 0;
      * backward, fp32 output: everything shows, at every fan-in."""
    fan_in = cin * k * k
    scale = WS_SCALE * fan_in ** -0.5
    w, gain = kc.standardize_rows(kind, cout, cin, k, seed=70)
    for khwc in (False, True):
        ref, bound = kc.weight_standardize_reference(w, gain, scale, WS_EPS, to_khwc=khwc)
        good = ws_stand_in(w, gain, scale, WS_EPS, to_khwc=khwc)
        worst = kc.assert_elementwise(good, ref, bound, f"honest weight_standardize {kind} {(cout, cin, k)} khwc={khwc}")
        assert worst < 1.0
    if kind == "constant":
        assert float(ref.abs().max()) == 0.0 and bool((good[0] == 0).all()) and bool((good[-1] == 0).all())
    else:
        check_fault("mean over ldo instead of the fan-in", ws_stand_in(w, gain, scale, WS_EPS, True, "mean over ldo", fan_in + 8), ref, bound)
    small = fan_in <= 216      # at fan-in 2048 the cancellation term gamma(n) |mean| of the bound is itself a few % of a 'large mean' row
    if kind == "large mean" and small:
        var = w.double().reshape(cout, -1).var(1, unbiased=False)
        assert float(var.max()) < 100 * WS_EPS          # var is of eps's size: where the place of eps matters
        check_fault("eps outside the root", ws_stand_in(w, gain, scale, WS_EPS, True, "eps outside the root"), ref, bound)
    if kind != "constant" and fan_in == 27:
        check_exceeds("unbiased variance (fan-in 27: 1.9 % of the value)", ws_stand_in(w, gain, scale, WS_EPS, True, "unbiased variance"), ref, bound)
    # backward
    g = torch.Generator().manual_seed(71)
    dwhat = torch.randn(cout, fan_in, generator=g)
    dw0, dg0 = torch.randn(cout, fan_in, generator=g), torch.randn(cout, generator=g)
    R = kc.weight_standardize_bwd_reference(w.reshape(cout, -1), gain, dwhat, scale, WS_EPS, 0.7, dw0, dg0)
    dw, dg = ws_bwd_stand_in(w, gain, dwhat, scale, WS_EPS, 0.7, dw0, dg0)
    assert kc.assert_elementwise(dw, *R["dw"], f"honest weight_standardize_bwd dw {kind} {(cout, cin, k)}") < 1.0
    assert kc.assert_elementwise(dg, *R["dgain"], f"honest weight_standardize_bwd dgain {kind} {(cout, cin, k)}") < 1.0
    j = int(R["dw"][0][-1].abs().argmax())          # in the last row, the element whose gradient is largest
    bad, _ = ws_bwd_stand_in(w, gain, dwhat, scale, WS_EPS, 0.7, dw0, dg0, "one gradient element dropped", drop=j)
    # 'large mean' at fan-in 2048: d_mean = gamma(2049) * 8 is 1.6 % of the one bf16 step that is the whole spread, and n inherits it
    (check_fault if small or kind != "large mean" else check_exceeds)("one element's gradient dropped", bad, *R["dw"])
    if kind == "normal" and small:  # 1 / (2 fan_in) of the value: at fan-in 2048 that is the size of the accumulation terms; a
        bad, badg = ws_bwd_stand_in(w, gain, dwhat, scale, WS_EPS, 0.7, dw0, dg0, "unbiased variance")   # constant row has var = 0 either way
        check_fault("unbiased variance (dw)", bad, *R["dw"])
        check_fault("unbiased variance (dgain)", badg, *R["dgain"])
    if kind == "large mean" and small:
        bad, _ = ws_bwd_stand_in(w, gain, dwhat, scale, WS_EPS, 0.7, dw0, dg0, "eps outside the root")
        check_fault("eps outside the root (dw)", bad, *R["dw"])


def test_weight_standardize_bwd_reference_is_the_gradient():
    """The closed form of the kernel's header against autograd through oracle.nfnet.standardized_weight, both in float64."""
    from oracle.nfnet import standardized_weight
    cout, cin, k = 12, 5, 3
    fan_in = cin * k * k
    w, gain = kc.standardize_rows("normal", cout, cin, k, seed=72)
    dwhat = rnd(cout, fan_in, seed=73)
    wd, gd = w.double().requires_grad_(True), gain.double().requires_grad_(True)
    flat = wd.reshape(cout, -1)                      # standardized_weight computes in float32: restate its lines in float64
    n = (flat - flat.mean(1, keepdim=True)) * torch.rsqrt(flat.var(1, unbiased=False, keepdim=True) + kc.f32_const(WS_EPS))
    sc = kc.f32_const(WS_SCALE * fan_in ** -0.5)
    what = n * gd.reshape(cout, 1) * sc
    assert torch.allclose(what.float(), standardized_weight(w.float(), gain.float(), WS_EPS).reshape(cout, -1) * (sc / (WS_SCALE * fan_in ** -0.5)), rtol=1e-5, atol=1e-6)
    (what * dwhat.double() * kc.f32_const(0.7)).sum().backward()
    R = kc.weight_standardize_bwd_reference(w.reshape(cout, -1), gain, dwhat, WS_SCALE * fan_in ** -0.5, WS_EPS, 0.7)
    assert torch.allclose(R["dw"][0], wd.grad.reshape(cout, -1), rtol=1e-11, atol=1e-13)
    assert torch.allclose(R["dgain"][0], gd.grad, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("HW", [1, 9, 33, 140])
def test_relu_mean_rows_stand_in_and_faults(HW):
    B, C = 3, 66
    x, g = kc.relu_rows_input(B, HW, C, seed=80 + HW)
    assert float(x[x > 0].min()) == 2.0 ** -133 and bool(torch.signbit(x[x == 0]).any()) and bool((~torch.signbit(x[x == 0])).any())
    ref, bound = kc.relu_mean_rows_reference(x)
    perm = torch.randperm(HW, generator=torch.Generator().manual_seed(5))
    s = torch.relu(x.float())[:, perm].sum(1)
    assert kc.assert_elementwise((s / HW).to(BF16), ref, bound, f"honest relu_mean_rows HW={HW}") < 1.0
    check_exceeds(f"relu_mean_rows: 1/(HW+1), HW={HW}", (s / (HW + 1)).to(BF16), ref, bound)
    rb, bb = kc.relu_mean_rows_bwd_reference(x, g)
    inv = torch.tensor(1.0, dtype=torch.float32) / HW
    good = torch.where(x.float() > 0, g.float()[:, None, :] * inv, torch.zeros(())).to(BF16)
    assert kc.assert_elementwise(good, rb, bb, f"honest relu_mean_rows_bwd HW={HW}") < 1.0
    assert bool((good[x <= 0] == 0).all()) and bool((good[x > 0] != 0).any())
    inv1 = torch.tensor(1.0, dtype=torch.float32) / (HW + 1)
    check_exceeds(f"relu_mean_rows_bwd: 1/(HW+1), HW={HW}", torch.where(x.float() > 0, g.float()[:, None, :] * inv1, torch.zeros(())).to(BF16), rb, bb)
    check_fault("relu_mean_rows_bwd: gate >= instead of >", torch.where(x.float() >= 0, g.float()[:, None, :] * inv, torch.zeros(())).to(BF16), rb, bb)
    bad = good.clone(); bad[-1, -1, -1] = 0 if float(good[-1, -1, -1]) != 0 else 1
    j = (x[-1, -1] > 0).nonzero().max()
    bad = good.clone(); bad[-1, -1, j] = 0
    check_fault("relu_mean_rows_bwd: one element's gradient dropped", bad, rb, bb)


def test_maxpool_bwd_reference_is_autograd():
    """kernel_compare.maxpool3x3s2_bwd_reference: its fp64 scatter through max_pool2d's own indices is autograd's backward (fp32)
    on a map with ties, and on a constant 5 x 7 map with dy = 1 it is the pattern of first valid window entries."""
    import torch.nn.functional as F
    x = torch.randint(-1, 2, (2, 8, 7, 9), generator=torch.Generator().manual_seed(1)).to(BF16)
    dy = rnd(2, 8, 4, 5, seed=2).to(BF16)
    xf = x.float().requires_grad_(True)
    F.max_pool2d(xf, 3, 2, 1).backward(dy.float())
    ref, bound, cnt = kc.maxpool3x3s2_bwd_reference(x, dy)
    assert torch.allclose(ref, xf.grad.double(), rtol=1e-6, atol=1e-7) and int(cnt.max()) >= 2
    ref, _, cnt = kc.maxpool3x3s2_bwd_reference(torch.full((1, 1, 5, 7), 0.5), torch.ones(1, 1, 3, 4))
    row = torch.tensor([1, 1, 0, 1, 0, 1, 0], dtype=torch.float64)
    want = torch.zeros(5, 7, dtype=torch.float64)
    want[0] = want[1] = want[3] = row
    assert torch.equal(ref[0, 0], want) and torch.equal(cnt[0, 0].double(), want)
    # a window of -inf gives its gradient to its first valid entry; a NaN takes it
    xi = torch.full((1, 1, 5, 7), float("-inf"))
    assert torch.equal(kc.maxpool3x3s2_bwd_reference(xi, torch.ones(1, 1, 3, 4))[0][0, 0], want)
    xi[0, 0, 2, 2] = float("nan")
    ref = kc.maxpool3x3s2_bwd_reference(xi, torch.ones(1, 1, 3, 4))[0][0, 0]
    assert float(ref[2, 2]) == 1.0 and float(ref[1, 1]) == 0.0 and float(ref.sum()) == 12.0


# ---------------------------------------------------------------------------------------------------------------------------
# the row kernels at their edges (tests/test_row_kernels_gpu.py): LayerNorm forward / backward and the cross-entropy head on the
# value families of kernel_compare.layernorm_family_rows / cross_entropy_family
# ---------------------------------------------------------------------------------------------------------------------------
LN_EPS = 1e-5


def ln_stats32(xf, fault=None):
    """mean, rstd of a row in float32, sums in a permuted order, with the seeded slips (all on the stand-in, never on a kernel)."""
    d = xf.shape[1]
    perm = torch.randperm(d, generator=torch.Generator().manual_seed(7))
    cols = perm[perm < d - 8] if fault == "mean over d - 8 elements" else perm     # the sum misses the last vector, the divisor is d
    mean = xf[:, cols].sum(-1, keepdim=True) / d
    var = ((xf - mean)[:, perm] ** 2).sum(-1, keepdim=True) / d
    rstd = torch.rsqrt(var) if fault == "eps dropped" else torch.rsqrt(var + LN_EPS)
    if fault == "statistics of the next row":
        mean, rstd = mean.roll(-1, 0), rstd.roll(-1, 0)
    return mean, rstd, perm


def ln_fwd_stand_in(x, g, b, fault=None):
    xf = x.float()
    mean, rstd, _ = ln_stats32(xf, fault)
    y = ((xf - mean) * rstd * g + b).to(BF16)
    if fault == "last 8-wide store dropped":
        y[-1, -8:] = float("nan")          # the GPU tests pre-fill every output with NaN: that is what a dropped store leaves
    return y


def ln_bwd_stand_in(dy, x, g, res, fault=None):
    xf = x.float()
    d = xf.shape[1]
    mean, rstd, perm = ln_stats32(xf, fault)
    xh = (xf - mean) * rstd
    gy = dy.float() * g
    c1 = gy[:, perm].sum(-1, keepdim=True) / d
    c2 = (gy * xh)[:, perm].sum(-1, keepdim=True) / d
    dx = rstd * (gy - c1 - xh * c2)
    if res is not None and fault != "res not added":
        dx = dx + res.float()
    dx, xh = dx.to(BF16), xh.to(BF16)
    if fault == "last 8-wide store dropped":
        dx[-1, -8:] = float("nan")
        xh[-1, -8:] = float("nan")
    return dx, xh


def ln_family_case(kind, rows, d):
    x = kc.layernorm_family_rows(kind, rows, d, seed=60)
    g = rnd(d, seed=61) * 0.1 + 1
    b = rnd(d, seed=62) * 0.1 + 0.25          # no beta near 0: an element that lost its store or its statistics shows
    dy = rnd(rows, d, seed=63).to(BF16)
    res = rnd(rows, d, seed=64).to(BF16)
    return x, g, b, dy, res


# What each seeded statistics fault must do to each family: the outputs ("fwd", "dx", "xhat") on which it must EXCEED the bound at
# both shapes, "no-op" where it cannot change a bit of any output, or a dict per d where the shape decides.  Every (family, fault)
# pair has an entry, and every output that is not listed to exceed is asserted to stay within the bound, so the table states
# the whole outcome and a change of either the bounds or the stand-in shows.
#   * rows of one family still differ (offset: the sample mean by 0.0625 / sqrt(d); constant: another c_r per row; spike: the
#     spike's column and the noise), so a row normalised with the NEXT row's statistics is outside the forward bound on every
#     family but the all-zero one.  On spike rows mean (200 / d) and variance of neighbours agree to ~1e-4: the shift of the
#     mean shows in the forward output (its small elements are ~ -mean * rstd, bound u_bf16 of that), while dx -- rstd times
#     terms that do not contain the mean -- moves by 1e-4 relative, inside the bf16 rounding;
#   * an all-zero row has mean 0 and variance 0 over any subset of any (all-zero) row: only the dropped eps can show (0 * inf);
#   * eps = 1e-5 against the variance: constant and zero rows (variance 0) divide by zero; spike rows (variance ~ 4e4 / d) move rstd
#     by a few fp32 ulps, nothing a bf16 output shows; offset rows (variance 0.0039): rstd moves by eps / (2 var) = 1.3e-3 relative, a third of u_bf16, within
#     the bound at d = 2056 -- and outside it at d = 8, where the three rows' sample variances are 2 to 4 times smaller.
NEXT_ROW, SHORT_MEAN, NO_EPS = "statistics of the next row", "mean over d - 8 elements", "eps dropped"
ALL3 = ("fwd", "dx", "xhat")
LN_STAT_FAULTS = {
    ("offset", NEXT_ROW): ALL3, ("offset", SHORT_MEAN): ALL3, ("offset", NO_EPS): {2056: (), 8: ALL3},
    ("constant", NEXT_ROW): ALL3, ("constant", SHORT_MEAN): ALL3, ("constant", NO_EPS): ALL3,
    ("spike", NEXT_ROW): {2056: ("fwd", "xhat"), 8: ("fwd",)}, ("spike", SHORT_MEAN): ALL3, ("spike", NO_EPS): (),
    ("zero", NEXT_ROW): "no-op", ("zero", SHORT_MEAN): "no-op", ("zero", NO_EPS): ALL3,
    ("mixed", NEXT_ROW): ALL3, ("mixed", SHORT_MEAN): ALL3, ("mixed", NO_EPS): ALL3,
}


@pytest.mark.parametrize("rows,d", [(5, 2056), (3, 8)])
@pytest.mark.parametrize("kind", kc.LN_FAMILIES + ("mixed",))
def test_layernorm_families_stand_in_and_faults(kind, rows, d):
    """Forward and backward bounds on the value families: the honest fp32 stand-in is inside (ratio printed), every seeded fault
    outside.  LN_STAT_FAULTS states, for every (family, statistics fault) pair, on which outputs the fault must exceed the bound,
    and where it cannot: there it is asserted to change nothing, or to stay within the bound."""
    x, g, b, dy, res = ln_family_case(kind, rows, d)
    T = kc.layernorm_terms(x, g, b, LN_EPS)
    ref, bound = T["ref"], kc.layernorm_bound(T, d)
    w = kc.assert_elementwise(ln_fwd_stand_in(x, g, b), ref, bound, f"honest LayerNorm, {kind} rows {rows}x{d}")
    assert w <= 1.0
    Rb = {r is not None: kc.layernorm_bwd_reference(dy, x, g, LN_EPS, res=r) for r in (res, None)}
    for with_res, r in ((True, res), (False, None)):
        dx, xh = ln_bwd_stand_in(dy, x, g, r)
        assert kc.assert_elementwise(dx, *Rb[with_res]["dx"], f"honest LayerNorm backward dx, {kind} rows {rows}x{d}, res {with_res}") <= 1.0
        assert kc.assert_elementwise(xh, *Rb[with_res]["xhat"], f"honest LayerNorm backward xhat, {kind} rows {rows}x{d}") <= 1.0
    honest = {"fwd": ln_fwd_stand_in(x, g, b)}
    honest["dx"], honest["xhat"] = ln_bwd_stand_in(dy, x, g, res)
    refs = {"fwd": (ref, bound), "dx": Rb[True]["dx"], "xhat": Rb[True]["xhat"]}
    for fault in (NEXT_ROW, SHORT_MEAN, NO_EPS):
        bad = {"fwd": ln_fwd_stand_in(x, g, b, fault)}
        bad["dx"], bad["xhat"] = ln_bwd_stand_in(dy, x, g, res, fault)
        want = LN_STAT_FAULTS[(kind, fault)]
        want = want[d] if isinstance(want, dict) else want
        for name in ALL3:
            what = f"{kind} {rows}x{d} {name}: {fault}"
            if want == "no-op":
                assert torch.equal(bad[name], honest[name]), f"{what}: expected to change nothing"
            elif name in want:
                check_exceeds(what, bad[name], *refs[name])
            else:
                w = kc.worst_ratio(bad[name], *refs[name])
                print(f"    fault {what:<58s} err/bound {w:9.3g}   (stated to stay within the bound)")
                assert w <= 1.0, f"{what}: {w:.3g}, LN_STAT_FAULTS states that this fault stays within the bound here"
    check_exceeds(f"{kind} {rows}x{d} forward: last 8-wide store dropped", ln_fwd_stand_in(x, g, b, "last 8-wide store dropped"), ref, bound)
    bad = ln_fwd_stand_in(x, g, b); bad[-1, -8:] = 0
    check_exceeds(f"{kind} {rows}x{d} forward: last 8 elements zero", bad, ref, bound)
    bdx, bxh = ln_bwd_stand_in(dy, x, g, res, "last 8-wide store dropped")
    check_exceeds(f"{kind} {rows}x{d} backward dx: last 8-wide store dropped", bdx, *Rb[True]["dx"])
    check_exceeds(f"{kind} {rows}x{d} backward xhat: last 8-wide store dropped", bxh, *Rb[True]["xhat"])
    bdx, _ = ln_bwd_stand_in(dy, x, g, res, "res not added")
    check_exceeds(f"{kind} {rows}x{d} backward dx: res not added", bdx, *Rb[True]["dx"])
    bdx, _ = ln_bwd_stand_in(dy, x, g, res)
    check_exceeds(f"{kind} {rows}x{d} backward dx: res added although none was given", bdx, *Rb[False]["dx"])


def ce_stand_in(lg, tg, fault=None, Vp=None, pad=1e30):
    """The three kernels in float32: maximum, exponentials, 256 strided partial sums, logarithm; the mean and the count over the
    rows whose target lies in [0, V); d logits rounded to bf16.  -> (rows, [mean, count], dlogits).  Seeded slips:
    "no max", "count includes out-of-range", "sum over V - 1", "sum over Vp" (pad columns hold ``pad``), "onehot at target + 1" / "- 1"."""
    x = lg.float()
    R, V = x.shape
    cols = x
    if fault == "sum over V - 1":
        cols = x[:, : V - 1]
    if fault == "sum over Vp":
        cols = torch.cat([x, torch.full((R, Vp - V), pad)], 1)
    mx = torch.zeros(R, 1) if fault == "no max" else cols.amax(1, keepdim=True)
    e = torch.exp(cols - mx)
    n = e.shape[1]
    part = torch.zeros(R, 256)
    for i in range(0, n, 256):                       # thread t adds columns t, t + 256, ... in order
        part[:, : min(256, n - i)] += e[:, i:i + 256]
    s = part.view(R, 4, 64).sum(-1).sum(-1, keepdim=True)
    valid = (tg >= 0) & (tg < V)
    t = torch.where(valid, tg, torch.zeros_like(tg))
    rows = torch.where(valid, (torch.log(s) + mx - x.gather(1, t[:, None])).squeeze(1), torch.zeros(R))
    counted = (tg >= 0) if fault == "count includes out-of-range" else valid
    cnt = counted.float().sum()
    mean = torch.where(counted, rows, torch.zeros(R)).sum() / cnt
    hot = t + (1 if fault == "onehot at target + 1" else -1 if fault == "onehot at target - 1" else 0)
    onehot = torch.zeros(R, V).scatter_(1, (hot % V)[:, None], 1.0)
    dl = (torch.exp(x - mx) * (1.0 / s) - onehot) * (1.0 / cnt)
    dl = torch.where(valid[:, None], dl, torch.zeros(R, V)).to(BF16)
    return rows, torch.stack([mean, cnt]), dl


def assert_ce(got, C, what):
    rows, stats, dl = got
    w = [kc.assert_elementwise(rows, *C["rows"], what + " row losses"), kc.assert_elementwise(dl, *C["dlogits"], what + " d logits")]
    if C["n_valid"]:
        w.append(kc.assert_elementwise(stats[:1], *C["mean"], what + " mean"))
    else:
        assert bool(torch.isnan(stats[0]))
    assert float(stats[1]) == C["n_valid"], f"{what}: count {float(stats[1])} != {C['n_valid']}"
    return max(w)


@pytest.mark.parametrize("V", [257, 50258])
@pytest.mark.parametrize("kind", kc.CE_FAMILIES)
def test_cross_entropy_families_stand_in(kind, V):
    lg, tg = kc.cross_entropy_family(kind, 5, V, seed=70)
    C = kc.cross_entropy_reference(lg, tg)
    assert assert_ce(ce_stand_in(lg, tg), C, f"honest cross-entropy, {kind} V={V}") <= 1.0
    if kind == "peaked":
        assert bool((C["rows"][0] == 0).all()) and bool((C["dlogits"][0] == 0).all())
    if kind == "peaked off":
        assert torch.allclose(C["rows"][0], torch.full((5,), 6e4, dtype=torch.float64))
    if kind == "flat":
        assert torch.allclose(C["rows"][0], torch.full((5,), math.log(V), dtype=torch.float64))


def test_cross_entropy_reference_ignores_targets_outside_the_vocabulary():
    """The contract the kernels are held to: -100 and every target outside [0, V) are ignored alike, and not counted."""
    V = 257
    lg, _ = kc.cross_entropy_family("gauss", 6, V, seed=71)
    tg = torch.tensor([3, 256, 257, 10 ** 6, -1, -100])
    C = kc.cross_entropy_reference(lg, tg)
    assert C["n_valid"] == 2 and C["n"] == 2
    two = torch.nn.functional.cross_entropy(lg[:2].double(), tg[:2], reduction="none")
    assert torch.allclose(C["rows"][0][:2], two, rtol=1e-12) and bool((C["rows"][0][2:] == 0).all())
    assert torch.allclose(C["mean"][0], two.mean().reshape(1), rtol=1e-12)
    lgr = lg[:2].double().requires_grad_(True)
    torch.nn.functional.cross_entropy(lgr, tg[:2]).backward()
    assert torch.allclose(C["dlogits"][0][:2], lgr.grad, rtol=1e-9, atol=1e-300) and bool((C["dlogits"][0][2:] == 0).all())
    assert bool((C["dlogits"][1][2:] <= kc.FLOOR).all()), "an ignored row has no allowance: exactly 0"
    assert assert_ce(ce_stand_in(lg, tg), C, "honest cross-entropy, targets outside [0, V)") <= 1.0
    rows, stats, dl = ce_stand_in(lg, tg, "count includes out-of-range")        # the kernel before the fix
    assert float(stats[1]) == 4
    check_exceeds("count includes the out-of-range rows: mean", stats[:1], *C["mean"])
    check_exceeds("count includes the out-of-range rows: d logits", dl, *C["dlogits"])


def test_cross_entropy_seeded_faults_exceed_the_bound():
    V, Vp = 257, 264
    lg, tg = kc.cross_entropy_family("peaked off", 5, V, seed=72)
    C = kc.cross_entropy_reference(lg, tg)
    rows, stats, dl = ce_stand_in(lg, tg, "no max")
    check_exceeds("peaked: no max subtraction, row losses", rows, *C["rows"])
    check_exceeds("peaked: no max subtraction, d logits", dl, *C["dlogits"])
    lg, tg = kc.cross_entropy_family("gauss", 5, V, seed=72)          # row 1: target V - 1; row 2: target at the arg-max
    lg[1, V - 1] = lg[1].max() + 1.0                                  # the last column carries most of row 1's sum
    C = kc.cross_entropy_reference(lg, tg)
    assert assert_ce(ce_stand_in(lg, tg), C, "honest cross-entropy, last column the largest") <= 1.0
    for fault in ("sum over V - 1", "sum over Vp"):
        rows, stats, dl = ce_stand_in(lg, tg, fault, Vp=Vp)
        check_exceeds(f"gauss: {fault}, row losses", rows, *C["rows"])
        check_exceeds(f"gauss: {fault}, d logits", dl, *C["dlogits"])
    for fault in ("onehot at target + 1", "onehot at target - 1"):
        for kind in kc.CE_FAMILIES[:4]:
            lg, tg = kc.cross_entropy_family(kind, 5, V, seed=72)
            rows, stats, dl = ce_stand_in(lg, tg, fault)
            check_exceeds(f"{kind}: {fault}", dl, *kc.cross_entropy_reference(lg, tg)["dlogits"])


# ---------------------------------------------------------------------------------------------------------------------------
# the 3x3 convolutions of the CLIP trunk (tests/test_conv_trunk_kernels_gpu.py): the new term builders against autograd, honest
# stand-ins that walk the operands the way the kernels do, and the seeded faults, in both input families at every table shape
# ---------------------------------------------------------------------------------------------------------------------------
CONV_IDS = [kc.conv_shape_id(s) for s in kc.CONV_SHAPES]
_conv_cases = {}


def conv_case(family, shape):
    """One set of operands and fp64 products per (family, shape), shared by the tests below and left unchanged."""
    key = (family, tuple(shape))
    if key not in _conv_cases:
        c = kc.conv_case(family, shape)
        c["fwd"] = kc.conv2d_terms(c["x"], c["w"])
        c["wd"] = kc.conv_dgrad_weight_rows(c["w"], c["scale"])
        c["dgrad"] = kc.conv2d_dgrad_terms(c["g"], wd=c["wd"])
        c["wgrad"] = kc.conv2d_wgrad_terms(c["g_rows"], c["x"])
        _conv_cases[key] = c
    return _conv_cases[key]


def conv_rows_stand_in(a_rows, wk, B, H, W, *, splits=1, fault=None):
    """The implicit-im2col GEMM as gemm128_kernel walks it, in fp32: a_rows [M, C] NHWC rows (bf16), wk [N, 9 C] (bf16) in
    (ky, kx, c) order.  K is walked in 16-byte chunks of 8 channels, 8 chunks per K-tile, ceil(K-tiles / splits) K-tiles per
    split; chunk q is tap q / cpt, channels 8 (q % cpt) ..; the A chunk of row m comes from row m + (ky - 1) W + (kx - 1) when
    that pixel is inside the image of m, and is zero for the halo and for tap >= 9.  Each split sums its own fp32 slab, the slabs
    are added in order.  -> fp32 [M, N].

    Seeded faults (one at a time):
      "halo_x"           the test on the column is left out: the neighbouring image row (or image) leaks in
      "halo_batch"       the test on the row is made on the row index of the whole batch: only the first and the last image
                         have a border above / below, every other border reads the neighbouring IMAGE
      "drop_last_ktile"  the last K-tile (the partial one where K % 64 != 0) is never staged
      "split_tap_floor"  a split's tap / channel counters start at the BEGINNING of the tap its first chunk lies in"""
    M, C = a_rows.shape
    N, K = wk.shape
    cpt, nkt = C // 8, -(-K // 64)
    kt_per = -(-nkt // splits)
    af = torch.cat([a_rows.float(), torch.zeros(1, C)])                      # row M: the zero page
    wp = torch.zeros(N, nkt * 64)
    wp[:, :K] = wk.float()
    m = torch.arange(M)
    xx, yy, row = m % W, (m // W) % H, m // W
    out = torch.zeros(M, N)
    for kt0 in range(0, nkt, kt_per):
        kt1 = min(nkt, kt0 + kt_per)
        if fault == "drop_last_ktile":
            kt1 = min(kt1, nkt - 1)
        if kt1 <= kt0:
            continue
        q = torch.arange(kt0 * 8, kt1 * 8)
        qa = q if fault != "split_tap_floor" else (kt0 * 8 // cpt) * cpt + (q - kt0 * 8)      # the chunk the A loader believes it is at
        tap, cc = qa // cpt, qa % cpt
        ky, kx = tap // 3, tap % 3
        y2, x2 = yy[:, None] + ky[None, :] - 1, xx[:, None] + kx[None, :] - 1
        ok = (tap < 9)[None, :] & (y2 >= 0) & (y2 < H) & (x2 >= 0) & (x2 < W)
        if fault == "halo_x":
            ok = (tap < 9)[None, :] & (y2 >= 0) & (y2 < H)
        if fault == "halo_batch":
            r2 = row[:, None] + ky[None, :] - 1
            ok = (tap < 9)[None, :] & (r2 >= 0) & (r2 < B * H) & (x2 >= 0) & (x2 < W)
        src = m[:, None] + (ky[None, :] - 1) * W + (kx[None, :] - 1)
        src = torch.where(ok & (src >= 0) & (src < M), src, torch.full_like(src, M))           # outside the tensor: nothing to leak
        a = af[src[:, :, None], (cc[None, :, None] * 8 + torch.arange(8)[None, None, :])]       # [M, chunks, 8]
        out += a.reshape(M, -1) @ wp[:, kt0 * 64: kt1 * 64].t()
    return out


def im2col_t_stand_in(x_rows, B, H, W, fault=None):
    """im2col_t_kernel tap by tap over the NHWC rows: out[ci * 9 + tap][m] = x_rows[m + (ky - 1) W + (kx - 1)][ci] inside the image,
    0 outside; the columns [M, round_up(M, 8)) are zero.  Fault "tail_copy": they hold a copy of column M - 1."""
    M, C = x_rows.shape
    Mp = -(-M // 8) * 8
    out = torch.zeros(C, 9, Mp, dtype=x_rows.dtype)
    m = torch.arange(M)
    xx, yy = m % W, (m // W) % H
    for tap in range(9):
        ky, kx = tap // 3, tap % 3
        ok = (yy + ky - 1 >= 0) & (yy + ky - 1 < H) & (xx + kx - 1 >= 0) & (xx + kx - 1 < W)
        src = (m + (ky - 1) * W + (kx - 1)).clamp(0, M - 1)
        out[:, tap, :M] = torch.where(ok[:, None], x_rows[src], torch.zeros_like(x_rows)).t()
    out = out.reshape(9 * C, Mp)
    if fault == "tail_copy":
        out[:, M:] = out[:, M - 1: M]
    return out


def transpose_stand_in(g_rows):
    M, C = g_rows.shape
    out = torch.zeros(C, -(-M // 8) * 8, dtype=g_rows.dtype)
    out[:, :M] = g_rows.t()
    return out


def wgrad_stand_in(gT, xT, base, scale, fault=None):
    """The accumulating fp32 GEMM of _acc_wgrad over round_up(M, 8) columns of both operands, in 64-column K-tiles:
    base + scale[co] * (gT xT^T).  Fault "row_scale_on_base": the factor is applied after the base was added."""
    acc = torch.zeros(gT.shape[0], xT.shape[0])
    for k0 in range(0, gT.shape[1], 64):
        acc += gT[:, k0:k0 + 64].float() @ xT[:, k0:k0 + 64].float().t()
    if fault == "row_scale_on_base":
        return (base + acc) * scale[:, None]
    return base + acc * scale[:, None]


def accepted(family, got, ref_bound) -> bool:
    """The verdict of the family's comparison: torch.equal with the reference cast once ("integers"), every element inside its
    bound ("gaussian")."""
    ref, bound = ref_bound
    if family == "integers":
        return torch.equal(got, ref.to(got.dtype))
    return kc.worst_ratio(got, ref, bound) <= 1.0


# the forward epilogue of the bottleneck with everything in it, and the dgrad epilogue of _unit_bwd's last call
def fwd_reference(c, full):
    if not full:
        return kc.epilogue_reference(c["fwd"])["C"]
    return kc.epilogue_reference(c["fwd"], scale=c["scale"], bias=c["bias"], act="relu", residuals=(c["res_out"],), act_after="relu")["C"]


def fwd_epilogue32(acc, c, full):
    if not full:
        return acc.to(BF16)
    v = torch.relu(acc * c["scale"] + c["bias"]) + c["res_out"].float()
    return torch.relu(v).to(BF16)


def dgrad_reference(c):
    return kc.epilogue_reference(c["dgrad"], aux=c["gate_in"], aux_mode="relu_gate", aux_after=True, residuals=(c["res_in"],))["C"]


def dgrad_epilogue32(acc, c):
    return ((acc + c["res_in"].float()) * (c["gate_in"].float() > 0)).to(BF16)


def wgrad_reference(c):
    return kc.epilogue_reference(c["wgrad"], row_scale=c["scale"], base=c["base"], out_dtype=torch.float32)["C"]


@pytest.mark.parametrize("shape", kc.CONV_SHAPES[:6], ids=CONV_IDS[:6])
def test_conv_term_builders_are_the_autograd_gradients(shape):
    """conv2d_dgrad_terms / conv2d_wgrad_terms (unfold + matmul in fp64) == fp64 autograd of F.conv2d(x, w * scale, padding = 1), and
    the dgrad terms taken from the re-laid-out operand == those taken from w and scale where w * scale is exact in bf16."""
    c = conv_case("integers", shape)
    B, H, W, Cin, Cout = shape
    x = c["x"].double().requires_grad_(True)
    w = c["w"].double().requires_grad_(True)
    ws = w * c["scale"].double().view(-1, 1, 1, 1)
    torch.nn.functional.conv2d(x, ws, padding=1).backward(c["g"].double())
    dx = x.grad.permute(0, 2, 3, 1).reshape(c["M"], Cin)
    ref, mag, K = kc.conv2d_dgrad_terms(c["g"], c["w"], c["scale"])
    assert K == 9 * Cout and torch.equal(ref, dx) and bool((mag >= ref.abs()).all())
    ref2, mag2, _ = c["dgrad"]
    assert torch.equal(ref2, dx) and torch.equal(mag2, mag)
    # dW of the SCALED weight is scale[co] * dW of the plain convolution: the row_scale of the wgrad GEMM
    dw, wmag, Kw = c["wgrad"]
    assert Kw == c["M"] and torch.equal(dw * c["scale"].double()[:, None], w.grad.reshape(Cout, 9 * Cin)) and bool((wmag >= dw.abs()).all())
    # gaussian operands: the same identities to fp64 rounding
    c = conv_case("gaussian", shape)
    x = c["x"].double().requires_grad_(True)
    w = c["w"].double().requires_grad_(True)
    torch.nn.functional.conv2d(x, w * c["scale"].double().view(-1, 1, 1, 1), padding=1).backward(c["g"].double())
    ref, mag, _ = kc.conv2d_dgrad_terms(c["g"], c["w"], c["scale"])
    assert float((ref - x.grad.permute(0, 2, 3, 1).reshape(c["M"], Cin)).abs().max()) <= 1e-12 * float(mag.max())
    dw, wmag, _ = c["wgrad"]
    assert float((dw * c["scale"].double()[:, None] - w.grad.reshape(Cout, 9 * Cin)).abs().max()) <= 1e-12 * float(wmag.max()) * 2.0


def test_integer_family_is_exact_in_fp32():
    """The premise of the "integers" family on the CPU: an fp32 convolution of such operands equals the fp64 one exactly, in two
    summation orders (a vendor convolution, and the tap-by-tap walk cut into three splits), and the magnitude sums stay below 2^23."""
    for shape in kc.CONV_SHAPES[:6]:
        c = conv_case("integers", shape)
        B, H, W, Cin, Cout = shape
        ref, mag, K = c["fwd"]
        assert kc.assert_exact_in_fp32(2.0 * mag + 16.0) <= 2.0 * 16 * 9 * Cin + 16
        f32 = torch.nn.functional.conv2d(c["x"].float(), c["w"].float(), padding=1).permute(0, 2, 3, 1).reshape(c["M"], Cout)
        assert torch.equal(f32.double(), ref)
        walked = conv_rows_stand_in(c["x_rows"], kc.conv_weight_rows(c["w"]), B, H, W, splits=3)
        assert torch.equal(walked.double(), ref) and torch.equal(walked.to(BF16), ref.to(BF16))
    with pytest.raises(AssertionError, match="no longer exact"):
        kc.assert_exact_in_fp32(torch.tensor([2.0 ** 23]))


def test_gemm128_splits_follows_the_dispatch_rules():
    """The split counts the GPU test asserts per case, spelled out: (M, N, K, split_k) -> slabs."""
    for (M, N, K, sk), want in {
        (1, 8, 72, 0): 1, (10, 16, 216, 0): 1, (105, 24, 360, 0): 1,                  # fewer than 8 K-tiles: no automatic split
        (270, 40, 648, 0): 2, (270, 40, 648, 2): 2, (270, 40, 648, 5): 4,             # 11 K-tiles: 6 + 5, and 3 + 3 + 3 + 2
        (144, 136, 1728, 0): 6, (144, 136, 1728, 2): 2, (144, 136, 1728, 5): 5,       # 27 K-tiles: 5 x 5 + 2, 14 + 13, 6 x 4 + 3
        (288, 768, 6912, 0): 16, (288, 768, 6912, 1): 1,                              # 108 K-tiles, 18 tiles: 15 x 7 + 3
        (270, 72, 360, 2): 2, (270, 72, 360, 5): 3, (144, 192, 1224, 0): 5,           # the dgrad calls (channels swapped)
    }.items():
        assert kc.gemm128_splits(M, N, K, sk) == want, (M, N, K, sk)
    # at cpt = 9 the splits of the forced 5-way request start at chunks 24, 48 and 72: two of them inside a tap
    assert kc.split_starts_inside_a_tap(648, 72, 4) == [24, 48]
    assert kc.split_starts_inside_a_tap(648, 72, 2) == [48]
    assert kc.split_starts_inside_a_tap(72, 8, 2) == []


# which seeded faults change nothing at a shape, and why -- asserted below instead of claimed
def vacuous(fault, shape):
    B, H, W, Cin, Cout = shape
    M = B * H * W
    if fault == "halo_x":
        return H * W == 1 and B == 1                 # no other pixel exists
    if fault == "halo_batch":
        return B == 1                                # no second image
    if fault == "no_flip":
        return H * W == 1                            # only the centre tap reaches a pixel, and the flip leaves it in place
    if fault == "drop_last_ktile":                   # every tap of the last K-tile is padding for every pixel: taps of the rows above /
        cpt, nkt = Cin // 8, -(-9 * Cin // 64)       # below in an image one pixel high, of the columns beside in one a pixel wide
        return all((H == 1 and t // 3 != 1) or (W == 1 and t % 3 != 1) for t in range((nkt - 1) * 8 // cpt, 9))
    if fault == "split_tap_floor":
        return not kc.split_starts_inside_a_tap(9 * Cin, Cin, 2)      # cpt = 1 or 2 (8 or 16 channels) divides the 8 chunks of a
                                                                      # K-tile: every split starts on a tap boundary
    if fault == "tail_copy":
        return M % 8 == 0                            # no tail columns
    return False


FWD_FAULTS = ("halo_x", "halo_batch", "drop_last_ktile", "split_tap_floor")


@pytest.mark.parametrize("family", kc.CONV_FAMILIES)
@pytest.mark.parametrize("shape", kc.CONV_SHAPES, ids=CONV_IDS)
def test_conv_forward_stand_in_and_faults(shape, family):
    c = conv_case(family, shape)
    B, H, W, Cin, Cout = shape
    wk = kc.conv_weight_rows(c["w"])
    for full in (False, True):
        ref = fwd_reference(c, full)
        for splits in (1, 2, 5):
            assert accepted(family, fwd_epilogue32(conv_rows_stand_in(c["x_rows"], wk, B, H, W, splits=splits), c, full), ref), (full, splits)
        honest = fwd_epilogue32(conv_rows_stand_in(c["x_rows"], wk, B, H, W, splits=2), c, full)
        for fault in FWD_FAULTS:
            bad = fwd_epilogue32(conv_rows_stand_in(c["x_rows"], wk, B, H, W, splits=2, fault=fault), c, full)
            if vacuous(fault, shape):
                assert torch.equal(bad, honest), f"{fault} was expected to change nothing at {shape}"
            else:
                assert not accepted(family, bad, ref), f"{fault} accepted at {shape}, {family}, full epilogue {full}"
    if family == "integers" and shape == (2, 9, 15, 72, 40):
        bad = conv_rows_stand_in(c["x_rows"], wk, B, H, W, fault="halo_x")
        frac = float((bad.double() != c["fwd"][0]).double().mean())
        print(f"    halo_x at {shape}: {100 * frac:.1f} % of the outputs change")
        assert frac > 0.05


@pytest.mark.parametrize("family", kc.CONV_FAMILIES)
@pytest.mark.parametrize("shape", kc.CONV_SHAPES, ids=CONV_IDS)
def test_conv_dgrad_stand_in_and_faults(shape, family):
    """The dgrad call: the same loader over the upstream gradient (Cout channels) against W' = the re-laid-out weight, gate and
    identity-path residual in the epilogue.  The loader's faults again, and the taps not flipped."""
    c = conv_case(family, shape)
    B, H, W, Cin, Cout = shape
    ref = dgrad_reference(c)
    for splits in (1, 2):
        assert accepted(family, dgrad_epilogue32(conv_rows_stand_in(c["g_rows"], c["wd"], B, H, W, splits=splits), c), ref), splits
    honest = dgrad_epilogue32(conv_rows_stand_in(c["g_rows"], c["wd"], B, H, W, splits=2), c)
    swapped = (B, H, W, Cout, Cin)                                      # the loader sees Cout channels here
    for fault in FWD_FAULTS + ("no_flip",):
        if fault == "no_flip":
            bad = conv_rows_stand_in(c["g_rows"], kc.conv_dgrad_weight_rows(c["w"], c["scale"], flip=False), B, H, W, splits=2)
        else:
            bad = conv_rows_stand_in(c["g_rows"], c["wd"], B, H, W, splits=2, fault=fault)
        bad = dgrad_epilogue32(bad, c)
        if vacuous(fault, swapped):
            assert torch.equal(bad, honest), f"{fault} was expected to change nothing at {shape}"
        else:
            assert not accepted(family, bad, ref), f"{fault} accepted at {shape}, {family}"


@pytest.mark.parametrize("family", kc.CONV_FAMILIES)
@pytest.mark.parametrize("shape", kc.CONV_SHAPES, ids=CONV_IDS)
def test_conv_wgrad_stand_in_and_faults(shape, family):
    c = conv_case(family, shape)
    B, H, W, Cin, Cout = shape
    M = c["M"]
    xT, gT = im2col_t_stand_in(c["x_rows"], B, H, W), transpose_stand_in(c["g_rows"])
    assert torch.equal(xT, kc.im2col_t_reference(c["x"]))
    ref = wgrad_reference(c)
    assert accepted(family, wgrad_stand_in(gT, xT, c["base"], c["scale"]), ref)
    assert not accepted(family, wgrad_stand_in(gT, xT, c["base"], c["scale"], fault="row_scale_on_base"), ref)
    # the tail columns: the layout check is what rejects a stale tail (the other operand's zeros hide it from the GEMM) ...
    bad = im2col_t_stand_in(c["x_rows"], B, H, W, fault="tail_copy")
    if vacuous("tail_copy", shape):
        assert torch.equal(bad, xT)
    else:
        assert not torch.equal(bad, kc.im2col_t_reference(c["x"])) and bool((bad[:, M:] != 0).any())
        # ... unless BOTH operands keep a stale tail: then the weight gradient itself is wrong
        gbad = gT.clone()
        gbad[:, M:] = gbad[:, M - 1: M]
        assert not accepted(family, wgrad_stand_in(gbad, bad, c["base"], c["scale"]), ref)


# ---------------------------------------------------------------------------------------------------------------------------
# the ViT attention backward (mg_attn_small_bwd_bf16)
# ---------------------------------------------------------------------------------------------------------------------------
ASB_GRADS = ("dq", "dk", "dv")
# fault -> the gradients it changes (D enters dS only; a scaled dQ / dK is that tensor alone)
ASB_FAULTS = {
    "8-wide store dropped in row S-1": ASB_GRADS,
    "8-wide store dropped in row S/2": ASB_GRADS,
    "row S-1 = the row above it": ASB_GRADS,
    "output sums end one index short": ASB_GRADS,
    "D omitted": ("dq", "dk"),
    "dq 2 % too large": ("dq",),
    "dk 2 % too large": ("dk",),
}
# A factor 1.02 cannot reach FAULT_FACTOR against a bf16 output, whatever the bound: the bound is at least u_bf16 |ref|, 2 % of a
# value is 0.02 / u_bf16 = 5.12 of that, and the output rounding of the scaled value moves it by at most 1.02 u_bf16 |ref| either
# way -- every ratio lies in [4.1, 6.14].  Among the elements of a tensor some round to the fault's side, so the worst one is
# above 5.12: that is what the table asserts for these two faults; all others must reach FAULT_FACTOR.
ASB_SCALE_FAULT_FLOOR = 0.02 / kc.U_BF16
ASB_OLD_TOL = 1e-2               # test_attn_small_backward: rel over the concatenated [dq | dk | dv] rows


def attn_small_bwd_stand_in(qkv, d_out, B, S, H, fault=None):
    """attn_small_bwd_kernel in fp32, step by step in its order: scores and dP as 64-term dot products, the row maximum,
    e = exp(t - m), l, inv = 1 / l, P = e inv, D = sum P dP, dS = P (dP - D) / 8, the three sums over S, one rounding to bf16.
    ``fault`` seeds what a mistake INSIDE the kernel would compute; faults of the stores are written into the result."""
    x = kc.heads_of(qkv.float(), B, S, H)
    q, k, v = x[0], x[1], x[2]
    dO = kc.heads_of(d_out.float(), B, S, H)[0]
    sc = (q @ k.transpose(-1, -2)) * 0.125
    dp = dO @ v.transpose(-1, -2)
    e = torch.exp(sc - sc.amax(-1, keepdim=True))
    p = e * (1.0 / e.sum(-1, keepdim=True))
    D = (p * dp).sum(-1, keepdim=True)
    if fault == "D omitted":
        D = torch.zeros_like(D)
    ds = p * (dp - D) * 0.125
    n = S - 1 if fault == "output sums end one index short" else S
    out = {"dq": ds[..., :n] @ k[..., :n, :], "dk": ds[..., :n, :].transpose(-1, -2) @ q[..., :n, :],
           "dv": p[..., :n, :].transpose(-1, -2) @ dO[..., :n, :]}
    if fault in ("dq 2 % too large", "dk 2 % too large"):
        out[fault[:2]] = out[fault[:2]] * 1.02
    out = {n_: t.to(BF16) for n_, t in out.items()}
    b, h = B - 1, H - 1
    for t in out.values():
        if fault == "8-wide store dropped in row S-1":
            t[b, h, S - 1, -8:] = 0
        elif fault == "8-wide store dropped in row S/2":
            t[b, h, S // 2, -8:] = 0
        elif fault == "row S-1 = the row above it":
            t[b, h, S - 1] = t[b, h, S - 2]
    return out


def asb_old_rel(got: dict, R: dict) -> float:
    """rel of test_attn_small_backward: over the concatenated [dq | dk | dv] rows (a Frobenius norm: the layout does not matter)."""
    num = sum(float((got[n].double() - R[n][0]).pow(2).sum()) for n in ASB_GRADS)
    return (num / sum(float(R[n][0].pow(2).sum()) for n in ASB_GRADS)) ** 0.5


@pytest.mark.parametrize("B,S,H", kc.ATTN_SMALL_BWD_SHAPES)
def test_attn_small_backward_stand_in_and_faults(B, S, H):
    """kernel_compare.attn_small_backward_reference at the shapes and input families of tests/test_vit_kernels_gpu.py:
      1. the honest fp32 stand-in is below 1 for dq, dk and dv on every family;
      2. every seeded fault (S > 1) reaches FAULT_FACTOR for each gradient it changes on at least one family, and on the
         "last key leads" family in particular (its gain is chosen for that: attn_small_lead_gain) -- except the 2 % faults,
         whose ceiling against a bf16 output is 6.14 (ASB_SCALE_FAULT_FLOOR);
      3. the 2 % faults are ACCEPTED by the whole-tensor rel < 1e-2 of test_attn_small_backward on that test's inputs."""
    table = {}
    cases = {}
    for family in kc.ATTN_SMALL_BWD_FAMILIES:
        qkv, d_out = kc.attn_small_backward_inputs(family, B, S, H)
        R = kc.attn_small_backward_reference(qkv, d_out, B, S, H)
        cases[family] = (qkv, d_out, R)
        good = attn_small_bwd_stand_in(qkv, d_out, B, S, H)
        for name in ASB_GRADS:
            w = kc.assert_elementwise(good[name], *R[name], f"honest attn_small backward {name}, B={B} S={S} H={H}, {family}")
            assert w < 1.0
            table[("honest", name, family)] = w
        assert asb_old_rel(good, R) < ASB_OLD_TOL
    print(f"  attn_small backward B={B} S={S} H={H}: worst err/bound per family {kc.ATTN_SMALL_BWD_FAMILIES}")
    for name in ASB_GRADS:
        print(f"    honest {name:<44s}" + "".join(f"{table[('honest', name, f)]:10.2f}" for f in kc.ATTN_SMALL_BWD_FAMILIES))
    if S == 1:
        for family, (qkv, d_out, R) in cases.items():          # one token: P = 1, dS = 0, dV = dO
            assert not R["dq"][0].any() and not R["dk"][0].any()
            assert torch.equal(R["dv"][0], kc.heads_of(d_out.double(), B, S, H)[0])
        return
    # "last key leads" is peaked on column S - 1 and not one-hot: the median largest weight of a row is at least 1/2 and sits on the
    # last key, and no row's exceeds 0.999 (a one-hot row has dS = 0: its dq row could be dropped unnoticed)
    x = kc.heads_of(cases["last key leads"][0].double(), B, S, H)
    top = torch.softmax(x[0] @ x[1].transpose(-1, -2) / 8.0, -1).max(-1)
    assert float(top.values.median()) >= 0.5 and float(top.values.max()) <= 0.999, (float(top.values.median()), float(top.values.max()))
    assert float((top.indices == S - 1).double().mean()) >= 0.99
    for fault, grads in ASB_FAULTS.items():
        scaled = fault.endswith("too large")
        need = ASB_SCALE_FAULT_FLOOR if scaled else FAULT_FACTOR
        bads = {f: attn_small_bwd_stand_in(qkv, d_out, B, S, H, fault=fault) for f, (qkv, d_out, R) in cases.items()}
        for name in grads:
            ws = {f: kc.worst_ratio(bads[f][name], *cases[f][2][name]) for f in cases}
            print(f"    {fault + ', ' + name:<51s}" + "".join(f"{ws[f]:10.4g}" for f in kc.ATTN_SMALL_BWD_FAMILIES))
            best = max(ws, key=ws.get)
            assert ws[best] >= need, f"{fault}, {name}: no family reaches {need:.2f} x the bound at B={B} S={S} H={H}: {ws}"
            assert ws["last key leads"] >= need, f"{fault}, {name}: 'last key leads' reaches only {ws['last key leads']:.2f}"
            with pytest.raises(AssertionError, match="bounding box"):
                kc.assert_elementwise(bads[best][name], *cases[best][2][name], f"{fault}, {name}, {best}")
        if scaled:
            old = asb_old_rel(bads["ViT scale"], cases["ViT scale"][2])
            print(f"    {fault + ': rel over [dq | dk | dv], ViT scale':<51s}{old:10.2e} < {ASB_OLD_TOL} (accepted before)")
            assert old < ASB_OLD_TOL, f"{fault}: the whole-tensor criterion was expected to accept it ({old:.3e})"


@pytest.mark.parametrize("B,S,H", [(2, 2, 1), (1, 7, 2), (2, 50, 3), (1, 64, 2)])
def test_attn_small_backward_reference_is_the_gradient(B, S, H):
    """The fp64 reference is torch.autograd through fp64 softmax(q k^T / 8) v, to 1e-12 of each gradient's largest element."""
    for family in ("i.i.d.", "last key leads"):
        qkv, d_out = kc.attn_small_backward_inputs(family, B, S, H)
        R = kc.attn_small_backward_reference(qkv, d_out, B, S, H)
        x = qkv.double().requires_grad_(True)
        q, k, v = kc.heads_of(x, B, S, H)
        o = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v
        o.backward(kc.heads_of(d_out.double(), B, S, H)[0])
        for name, grad in zip(ASB_GRADS, kc.heads_of(x.grad, B, S, H)):
            err = float((R[name][0] - grad).abs().max() / grad.abs().max())
            assert err <= 1e-12, (name, family, err)
