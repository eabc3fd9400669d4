"""The named epilogue configurations of the GEMM tests, their inputs, and an fp32 stand-in of the contract -- shared by
tests/test_kernel_compare_cpu.py (stand-in and seeded faults, no GPU) and tests/test_gemm_epilogue_matrix_gpu.py (every GEMM path).

Plain module, imported the way kernel_compare.py is: no fixtures, no pytest settings.

A configuration says WHICH fields of mg_epilogue (include/magma_hip.h) are set; tensors are made for a shape by ``make_case``.
The list is not a cross product.  It holds
  * every combination the engines issue (``site`` = the call), and
  * "cover" entries that put an activation, an aux mode and most other fields together, so that every pair of
    {scale, row_scale, bias, act in 4, act_n0, aux_mode in 5, aux_after, residual count 1..3, act_after, C2, fp32 output,
    accumulate} the library accepts occurs in one entry at least (test_epilogue_configurations_cover_every_pair).
It has 40 entries: the engines alone issue 28 distinct combinations and the 12 activation x aux-mode pairs need an entry each."""
import torch

import kernel_compare as kc

BF16 = torch.bfloat16


def cfg(name, site, *, scale=False, row_scale=False, bias=False, act="none", act_n0=False, aux_mode="none", aux_after=False,
        n_res=0, act_after=False, c2=False, out_f32=False, accumulate=False):
    assert act in kc.ACTS and aux_mode in kc.AUX_MODES and 0 <= n_res <= 3
    assert not accumulate or out_f32, "accumulate adds into an fp32 output (check_epilogue)"
    assert not act_n0 or act != "none"
    assert not aux_after or aux_mode != "none"
    return dict(name=name, site=site, scale=scale, row_scale=row_scale, bias=bias, act=act, act_n0=act_n0, aux_mode=aux_mode,
                aux_after=aux_after, n_res=n_res, act_after=act_after, c2=c2, out_f32=out_f32, accumulate=accumulate)


CONFIGS = [
    # ---- what the engines issue ----------------------------------------------------------------------------------------
    cfg("plain", "engine.py:_linear without options; train_engine.py:847 (dgrad without bias)"),
    cfg("bias", "engine.py:_linear (qkv, lm_head)", bias=True),
    cfg("bias_f32", "engine.py lm_head logits (fp32 output)", bias=True, out_f32=True),
    cfg("bias_gelu", "engine.py:605,884 fc_in", bias=True, act="gelu"),
    cfg("bias_gelu_n0", "engine.py:588 [q|k|v | fc_in] in one launch", bias=True, act="gelu", act_n0=True),
    cfg("bias_gelu_c2", "train_engine.py:698 fc_in with the saved pre-activation", bias=True, act="gelu", c2=True),
    cfg("bias_relu", "engine.py:607,901 adapter down", bias=True, act="relu"),
    cfg("bias_relu_c2", "train_engine.py:559 adapter down with the saved pre-activation", bias=True, act="relu", c2=True),
    cfg("bias_quick_gelu", "image_encoders.py:248 CLIP ViT c_fc", bias=True, act="quick_gelu"),
    cfg("bias_quick_gelu_c2", "train_engine.py:1215 CLIP ViT c_fc with the saved pre-activation", bias=True, act="quick_gelu", c2=True),
    cfg("bias_res1", "image_encoders.py:246,249; train_engine.py:1212,1216; engine.py:619", bias=True, n_res=1),
    cfg("bias_res2", "engine.py:608,631,902,984; train_engine.py:707,730", bias=True, n_res=2),
    cfg("bias_res3", "engine.py:629,928,945,980; train_engine.py:727", bias=True, n_res=3),
    cfg("scale_bias_res1", "engine.py:616,963; train_engine.py:690 scaled adapter up", scale=True, bias=True, n_res=1),
    cfg("scale_bias_res3", "engine.py:625,977 (the decode step); train_engine.py:713", scale=True, bias=True, n_res=3),
    cfg("scale_bias_relu", "image_encoders.py:125; train_engine.py:1359 folded BatchNorm + ReLU", scale=True, bias=True, act="relu"),
    cfg("scale_bias_res1_relu_after", "image_encoders.py:126; train_engine.py:1361 bottleneck tail", scale=True, bias=True, n_res=1, act_after=True),
    cfg("scale_bias_relu_res1", "image_encoders.py:367; train_engine.py:1088 NF-ResNet unit", scale=True, bias=True, act="relu", n_res=1),
    cfg("res1", "train_engine.py:818,962 dgrad plus a residual gradient", n_res=1),
    cfg("gate", "train_engine.py:808,1020,1126 ReLU backward in the dgrad GEMM", aux_mode="relu_gate"),
    cfg("gate_res1", "train_engine.py:1125,1460 conv backward", aux_mode="relu_gate", n_res=1),
    cfg("gate_after_res1", "train_engine.py:1495 bottleneck tail backward (gate_after)", aux_mode="relu_gate", aux_after=True, n_res=1),
    cfg("gelu_grad", "train_engine.py:808,925 GELU backward in the dgrad GEMM", aux_mode="gelu_grad"),
    cfg("scale_gelu_grad", "train_engine.py:850 scaled adapter, GELU backward", scale=True, aux_mode="gelu_grad"),
    cfg("quick_gelu_grad", "train_engine.py:1238 CLIP ViT MLP backward", aux_mode="quick_gelu_grad"),
    cfg("bias_mul", "image_prefix.py:80; train_engine.py:994 dropout mask", bias=True, aux_mode="mul"),
    cfg("acc_row_scale_f32", "train_engine.py:791,1446 weight gradients accumulate in place", row_scale=True, out_f32=True, accumulate=True),
    cfg("acc_f32", "train_engine.py:791 weight gradients without a row scale", out_f32=True, accumulate=True),
    # ---- cover entries: activation x aux mode, the other fields spread over them --------------------------------------------
    cfg("cover_relu_gate", "cover", row_scale=True, scale=True, bias=True, act="relu", act_n0=True, aux_mode="relu_gate",
        aux_after=True, n_res=3, act_after=True, c2=True, out_f32=True, accumulate=True),
    cfg("cover_relu_gelu_grad", "cover", scale=True, bias=True, act="relu", aux_mode="gelu_grad", n_res=2, c2=True),
    cfg("cover_relu_mul", "cover", row_scale=True, bias=True, act="relu", aux_mode="mul", aux_after=True, n_res=1, act_after=True, out_f32=True),
    cfg("cover_relu_quick_grad", "cover", bias=True, act="relu", act_n0=True, aux_mode="quick_gelu_grad", n_res=3, act_after=True),
    cfg("cover_gelu_gate", "cover", scale=True, bias=True, act="gelu", aux_mode="relu_gate", n_res=2, act_after=True, c2=True),
    cfg("cover_gelu_gelu_grad", "cover", row_scale=True, scale=True, bias=True, act="gelu", act_n0=True, aux_mode="gelu_grad",
        aux_after=True, n_res=3, act_after=True, c2=True, out_f32=True, accumulate=True),
    cfg("cover_gelu_mul", "cover", bias=True, act="gelu", act_n0=True, aux_mode="mul", n_res=1, c2=True, out_f32=True),
    cfg("cover_gelu_quick_grad", "cover", row_scale=True, bias=True, act="gelu", aux_mode="quick_gelu_grad", aux_after=True, n_res=2),
    cfg("cover_quick_gate", "cover", row_scale=True, bias=True, act="quick_gelu", act_n0=True, aux_mode="relu_gate", n_res=1, c2=True),
    cfg("cover_quick_gelu_grad", "cover", scale=True, bias=True, act="quick_gelu", aux_mode="gelu_grad", aux_after=True, n_res=1, out_f32=True),
    cfg("cover_quick_mul", "cover", row_scale=True, scale=True, bias=True, act="quick_gelu", act_n0=True, aux_mode="mul",
        aux_after=True, n_res=3, act_after=True, c2=True, out_f32=True, accumulate=True),
    cfg("cover_quick_quick_grad", "cover", row_scale=True, scale=True, bias=True, act="quick_gelu", act_n0=True,
        aux_mode="quick_gelu_grad", aux_after=True, n_res=3, act_after=True, c2=True, out_f32=True, accumulate=True),
]
BY_NAME = {c["name"]: c for c in CONFIGS}
assert len(BY_NAME) == len(CONFIGS)


def features(c) -> set:
    """The 'on' values of a configuration, one name each: what test_epilogue_configurations_cover_every_pair counts."""
    f = {k for k in ("scale", "row_scale", "bias", "act_n0", "aux_after", "act_after", "c2", "out_f32", "accumulate") if c[k]}
    if c["act"] != "none":
        f.add("act=" + c["act"])
    if c["aux_mode"] != "none":
        f.add("aux=" + c["aux_mode"])
    if c["n_res"]:
        f.add("res")
    return f


def act_n0_of(N: int) -> int:
    """First activated column of the act_n0 configurations at width N: a multiple of 8 near the middle, inside a tile."""
    return (N // 2) // 8 * 8 + 8


# rows / columns at the corners of the 64-row wave blocks and 8-column lane groups of the tile kernels
CORNER_ROWS = (0, 63, 64, 127, 128, -1)
CORNER_COLS = (0, 7, 8, -1)
BIG = 30.0          # |aux| at which both GELU derivatives have reached 1 (+) and 0 (-)


def corner_index(M: int, N: int):
    rows = sorted({r % M for r in CORNER_ROWS if -M <= r < M})
    cols = sorted({c % N for c in CORNER_COLS if -N <= c < N})
    return rows, cols


def big_index(M: int, N: int):
    """((row, col) of aux = +BIG, (row, col) of aux = -BIG): off the corner rows / columns."""
    return (min(1, M - 1), 1), (min(2, M - 1), 2)


def make_case(M: int, N: int, K: int, seed: int = 0, device="cpu", with_product: bool = True) -> dict:
    """Every operand a configuration may use, for an M x N x K problem, made on the host from ``seed`` and moved to ``device``.
    The accumulator has a standard deviation of about 1 (a ~ N(0, 1), w ~ N(0, 1 / K)); bias, residuals and base are N(0, 1) too, so
    that one of them missing or misplaced moves an element by about its own size.  scale, row_scale: 0.5 + |N(0, 1)|.
    aux: N(0, 1) in bf16 with
      * exact 0.0 on every 7th and exact -0.0 on every 11th element (row-major), so that a gate ``>=`` differs from ``>`` on a
        fixed share of the tensor;
      * 0.0 / -0.0 alternating on the tile-corner positions (corner_index);
      * +BIG and -BIG at big_index."""
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    c = dict(M=M, N=N, K=K)
    if with_product:
        c["a"] = r(M, K).to(BF16)
        c["w"] = (r(N, K) * K ** -0.5).to(BF16)
    c["bias"] = r(N)
    c["scale"] = r(N).abs() + 0.5
    c["row_scale"] = r(M).abs() + 0.5
    c["res"] = [r(M, N).to(BF16) for _ in range(3)]
    c["base"] = r(M, N)
    aux = r(M, N).to(BF16)
    flat = aux.view(-1)
    flat[::7] = 0.0
    flat[::11] = -0.0
    rows, cols = corner_index(M, N)
    for i, rr in enumerate(rows):
        for j, cc in enumerate(cols):
            aux[rr, cc] = 0.0 if (i + j) % 2 == 0 else -0.0
    (rp, cp), (rn, cn) = big_index(M, N)
    aux[rp, cp], aux[rn, cn] = BIG, -BIG
    c["aux"] = aux
    return {k: (v.to(device) if torch.is_tensor(v) else ([t.to(device) for t in v] if isinstance(v, list) else v)) for k, v in c.items()}


def reference(case: dict, c: dict, prod_terms=None, *, fp8_scales: bool = False) -> dict:
    """kernel_compare.epilogue_reference of configuration ``c`` on the operands of ``case``.  prod_terms replaces the bf16 product
    (convolution, fp8).  fp8_scales: the caller's prod_terms belong to mg_gemm_fp8, whose row and column scales come from the
    quantiser: ``case`` then holds them as row_scale / scale and they are applied whatever ``c`` says."""
    if prod_terms is None:
        p, m = kc.product_terms(case["a"], case["w"])
        prod_terms = (p, m, case["K"])
    N = case["N"]
    return kc.epilogue_reference(
        prod_terms,
        scale=case["scale"] if (c["scale"] or fp8_scales) else None,
        row_scale=case["row_scale"] if (c["row_scale"] or fp8_scales) else None,
        bias=case["bias"] if c["bias"] else None,
        act=c["act"], act_n0=act_n0_of(N) if c["act_n0"] else 0,
        aux=case["aux"] if c["aux_mode"] != "none" else None, aux_mode=c["aux_mode"], aux_after=c["aux_after"],
        residuals=case["res"][: c["n_res"]], act_after="relu" if c["act_after"] else "none",
        base=case["base"] if c["accumulate"] else None,
        out_dtype=torch.float32 if c["out_f32"] else BF16)


def closed_gate_expectation(case: dict, c: dict) -> torch.Tensor:
    """What a relu_gate configuration must store where aux is 0.0 or -0.0, EXACTLY (fp32 of the kernel's own operations, then the
    output type): the gate closes, so with the gate before the residuals the output is res0 + res1 + res2 added in that order
    to 0 (then the trailing ReLU, then ``base +`` when accumulating); with aux_after it is 0 (resp. base).  Whole [M, N]
    tensor; the caller looks at the positions where aux == 0."""
    assert c["aux_mode"] == "relu_gate"
    v = torch.zeros(case["M"], case["N"], dtype=torch.float32, device=case["aux"].device)
    if not c["aux_after"]:
        for r in case["res"][: c["n_res"]]:
            v = v + r.float()
    if c["act_after"]:
        v = torch.relu(v)
    if c["accumulate"]:
        v = case["base"] + v
    return v if c["out_f32"] else v.to(BF16)


# ---------------------------------------------------------------------------------------------------------------------------
# the honest fp32 stand-in of the contract, and the faults a hand-written copy of it can have
# ---------------------------------------------------------------------------------------------------------------------------
FAULTS = ("aux on the wrong side of the residuals", "activation left of act_n0", "C2 taken after the activation",
          "res2 dropped in the last N % 8 columns", "gate with >=", "row_scale after the bias", "trailing ReLU skipped",
          "accumulate overwrites")


def fault_applies(fault: str, c: dict, N: int) -> bool:
    return {
        "aux on the wrong side of the residuals": c["aux_mode"] != "none" and c["n_res"] > 0,
        "activation left of act_n0": c["act_n0"],
        "C2 taken after the activation": c["c2"] and c["act"] != "none",
        "res2 dropped in the last N % 8 columns": c["n_res"] == 3 and N % 8 != 0,
        "gate with >=": c["aux_mode"] == "relu_gate",
        "row_scale after the bias": c["row_scale"] and c["bias"],
        "trailing ReLU skipped": c["act_after"],
        "accumulate overwrites": c["accumulate"],
    }[fault]


def _act32(v, act):
    if act == "relu":
        return torch.relu(v)
    if act == "gelu":        # gelu_new_f of csrc/common.h
        k0, k1 = 0.7978845608028654, 0.044715
        u = k0 * (v + k1 * v * v * v)
        return v * (1.0 / (1.0 + torch.exp(-2.0 * u)))
    if act == "quick_gelu":
        return v * (1.0 / (1.0 + torch.exp(-1.702 * v)))
    return v


def _aux32(a, mode, gate_ge=False):
    if mode == "relu_gate":
        return ((a >= 0) if gate_ge else (a > 0)).float()
    if mode == "mul":
        return a
    if mode == "gelu_grad":  # gelu_new_grad_f
        k0, k1 = 0.7978845608028654, 0.044715
        sg = 1.0 / (1.0 + torch.exp(-2.0 * k0 * (a + k1 * a * a * a)))
        t = 2.0 * sg - 1.0
        return sg + 0.5 * a * (1.0 - t * t) * k0 * (1.0 + 3.0 * k1 * a * a)
    sg = 1.0 / (1.0 + torch.exp(-1.702 * a))      # quick_gelu_grad_f
    return sg * (1.0 + 1.702 * a * (1.0 - sg))


def stand_in(case: dict, c: dict, fault: str = None, seed: int = 9):
    """(C, C2) of configuration ``c`` in plain float32 torch on the host, rounding where the kernels round: the product summed over
    64-wide chunks of a permuted K, every epilogue step one fp32 operation, C2 and a bf16 C rounded once.  ``fault``: one of FAULTS,
    written into the arithmetic the way a slip in a hand-written copy would be."""
    assert fault is None or fault in FAULTS
    M, N, K = case["M"], case["N"], case["K"]
    af, wf = case["a"].float(), case["w"].float()
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(seed))
    v = torch.zeros(M, N, dtype=torch.float32)
    for ch in perm.split(64):
        v += af[:, ch] @ wf[:, ch].t()
    late_rs = fault == "row_scale after the bias"
    if c["row_scale"] and not late_rs:
        v = v * case["row_scale"][:, None]
    if c["scale"]:
        v = v * case["scale"]
    if c["bias"]:
        v = v + case["bias"]
    if c["row_scale"] and late_rs:
        v = v * case["row_scale"][:, None]
    pre = v
    if c["act"] != "none":
        y = _act32(v, c["act"])
        if c["act_n0"] and fault != "activation left of act_n0":
            y = torch.where(torch.arange(N) >= act_n0_of(N), y, v)
        v = y
    c2 = (v if fault == "C2 taken after the activation" else pre).to(BF16)
    aux_after = c["aux_after"] != (fault == "aux on the wrong side of the residuals")
    f = _aux32(case["aux"].float(), c["aux_mode"], gate_ge=fault == "gate with >=") if c["aux_mode"] != "none" else None
    if f is not None and not aux_after:
        v = v * f
    for i, r in enumerate(case["res"][: c["n_res"]]):
        rf = r.float()
        if i == 2 and fault == "res2 dropped in the last N % 8 columns":
            rf = rf.clone()
            rf[:, N - N % 8:] = 0
        v = v + rf
    if f is not None and aux_after:
        v = v * f
    if c["act_after"] and fault != "trailing ReLU skipped":
        v = torch.relu(v)
    if c["accumulate"] and fault != "accumulate overwrites":
        v = case["base"] + v
    return (v if c["out_f32"] else v.to(BF16)), c2
