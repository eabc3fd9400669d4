"""One epilogue contract, four hand-written copies: every GEMM path against kernel_compare.epilogue_reference.

mg_epilogue (include/magma_hip.h) is implemented in epilogue_apply, the two-row block of epilogue_rows_c, the fast path of
epilogue_store4 and its fall-back into epilogue_apply<4> (magma_amd/csrc/gemm_device.h).  Here the named configurations of
tests/epilogue_cases.py run through every path that reaches one of them, at the smallest shape that reaches the code.  Which
build a shape selects follows from gemm_dispatch / gemm256_kernel / epilogue_rows (magma_amd/csrc/gemm.hip, gemm_device.h):

  path                      shape (M x N x K)           build
  128x128 wide              130 x 264 x 128             epilogue_rows<128, W = 8>; two-row block on the lanes with n + 8 <= N (all of
                                                        them: N % 8 == 0), LOADS = false when no aux / residual / accumulate; row
                                                        tiles 0..127 and 128..129, column tiles 0..127, 128..255, 256..263
  128x128 per-element tail  130 x 203 x 128             the lane at n = 200 has 3 of its 8 columns inside: epilogue_apply<8> tail code
  128x128 narrow            130 x 264 x 128             one of ldc / ldr / ldaux / ldc2 = 4 (mod 8): epilogue_wide_ok false, W = 4
  256x256                   300 x 520 x 256, tile=256   column tiles 0 and 256 interior (W = 8, FULL; LOADS = false without aux /
                                                        residual / accumulate), column tile 512 the (W = 8, edge) build with 8 columns;
                                                        row tile 256..299 cut at M
  256x256 per-element tail  300 x 523 x 256, tile=256   the lane at n = 520 of the edge tile holds 3 of 8 columns: the tail code of
                                                        epilogue_apply<8>, reached from the 256x256 kernel
  256x256 narrow            300 x 520 x 256             the (W = 4, edge) build on every column tile
  256x256 non-temporal      4096 x 4096 x 128 fp32,     gp.nt (output >= 64 MiB): (W = 8, NT, FULL), and (W = 8, NT, edge) on the
                            4096 x 8192|8200 x 128 bf16 last column tile at N = 8200
  split-K 128               200 x 203 x 1024, 4 splits  splitk_fixup_kernel -> epilogue_store4: fast path on whole quads without aux /
                                                        C2, epilogue_apply<4> otherwise and on the quad at n = 200 (3 columns)
  split-K 256               512 x 520 x 2048, 2 splits  the same fix-up over the 256 kernel's slabs (ldws = 768)
  conv3x3                   2 x 12 x 10, 16 -> 24       128x128 kernel, implicit-im2col A loader (M = 240, N = 24, K = 144)
  fp8 / MX, tiles 128, 256  300 x 512 x 256             the same walks with the activation row scale as the kernel argument
                                                        (mg_gemm_fp8) or no scales (mg_gemm_mx_fp8); Q8 build for the C8 copy
  skinny                    M 1 | 16, N 208 | 203,      skinny_body -> epilogue_store4 (4 waves x 1 k-step: K = 512 has 16 k-steps);
                            K = 512                     aux / C2 and the quad at n = 200 take epilogue_apply<4>
  skinny split_n            N = 208 + 203               ep for the columns < 208, ep_b for the rest (tail inside ep_b)
  skinny2, attention+GEMV   K = 512                     skinny2_kernel<4, 1, 1>, decode_attn_gemv_kernel<4>

Per case: C (and C2) per element against the fp64 restatement; the same bits from a second run, from the narrow and the wide walk,
with and without C2 (which moves a split-K or GEMV case between the fast and the general path), and from the LOADS = false build and
the LOADS = true build (reached through a residual of zeros); every output lives in a buffer of M + 3 rows and padded columns
prefilled with a sentinel, which must survive outside [0, M) x [0, N); where a ReLU gate is closed (aux = 0.0 / -0.0, placed on the
tile corners) the output is exactly the residual sum; at aux = +30 / -30 the GELU-gradient factor is exactly 1 / 0."""
import pytest
import torch

import epilogue_cases as ec
import kernel_compare as kcmp

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SENT = 7.0              # exact in bf16 and fp32; the outputs are N(0, few): an element equal to it by chance still passes
SENT8 = 0x5A
ALL = [c["name"] for c in ec.CONFIGS]


def codes(ops, c):
    act = {"none": ops.MG_ACT_NONE, "relu": ops.MG_ACT_RELU, "gelu": ops.MG_ACT_GELU_NEW, "quick_gelu": ops.MG_ACT_QUICK_GELU}
    aux = {"none": ops.MG_AUX_NONE, "relu_gate": ops.MG_AUX_RELU_GATE, "gelu_grad": ops.MG_AUX_GELU_GRAD, "mul": ops.MG_AUX_MUL,
           "quick_gelu_grad": ops.MG_AUX_QUICK_GELU_GRAD}
    return act[c["act"]], aux[c["aux_mode"]]


def ceil8(n):
    return (n + 7) // 8 * 8


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    it = torch.int16 if a.dtype == BF16 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# one problem (operands, packed weight, fp64 product) is kept at a time: the items of one path follow each other
_problem = {}


def problem(dev, M, N, K, seed=0, make=None):
    key = (M, N, K, seed, make is not None)
    if _problem.get("key") != key:
        _problem.clear()
        torch.cuda.empty_cache()
        from magma_amd import ops
        case = ec.make_case(M, N, K, seed=seed, device=dev, with_product=make is None)
        if make is None:
            case["lin"] = ops.PackedLinear(case["w"], bias=case["bias"], tiled=True, rowmajor=True)
            p, m = kcmp.product_terms(case["a"], case["w"])
            case["prod"] = (p, m, K)
        else:
            make(case)
        _problem.update(key=key, case=case)
    return _problem["case"]


def padded(t, ld, rows_extra=0, fill=SENT):
    """t [M, N] inside a [M + rows_extra, ld] buffer of ``fill`` -> (buffer, view)."""
    M, N = t.shape
    buf = torch.full((M + rows_extra, ld), fill, dtype=t.dtype, device=t.device)
    buf[:M, :N] = t
    return buf, buf[:M, :N]


def assert_sentinels(buf, M, N, what, fill=SENT):
    assert bool((buf[M:] == fill).all()), f"{what}: wrote to rows >= M"
    assert bool((buf[:M, N:] == fill).all()), f"{what}: wrote to columns >= N"


def epilogue_kwargs(ops, case, c, ld=None, zero_residual=False):
    """Keyword arguments of ops.gemm / gemm_fp8 / gemm_mx_fp8 / gemm_skinny for configuration ``c`` with every output in a sentinel
    buffer -> (kwargs, buffers to check afterwards).  ld: leading dimensions by operand ('c', 'r', 'aux', 'c2'); default
    ceil8(N) + 8 (a multiple of 8: the wide walk).  zero_residual: one residual of zeros more than ``c`` asks for."""
    M, N = case["M"], case["N"]
    ld = dict(ld or {})
    wide = ceil8(N) + 8
    dt = torch.float32 if c["out_f32"] else BF16
    dev = case["aux"].device
    init = case["base"] if c["accumulate"] else torch.full((M, N), SENT, dtype=dt, device=dev)
    cbuf, cview = padded(init.to(dt), ld.get("c", wide), 3)
    act, aux_mode = codes(ops, c)
    kw = dict(out=cview, act=act, act_after=ops.MG_ACT_RELU if c["act_after"] else ops.MG_ACT_NONE, use_bias=c["bias"])
    res = [padded(r, ld.get("r", wide))[1] for r in case["res"][: c["n_res"]]]
    if zero_residual:
        res.append(padded(torch.zeros(M, N, dtype=BF16, device=dev), ld.get("r", wide))[1])
    kw["residuals"] = tuple(res)
    if c["aux_mode"] != "none":
        kw.update(aux=padded(case["aux"], ld.get("aux", wide))[1], aux_mode=aux_mode, aux_after=c["aux_after"])
    bufs = {"C": cbuf}
    if c["c2"]:
        bufs["C2"], kw["out2"] = padded(torch.full((M, N), SENT, dtype=BF16, device=dev), ld.get("c2", wide), 3)
    return kw, bufs


def run_gemm(ops, case, c, *, tile=0, split_k=1, ld=None, zero_residual=False, layout="ft", conv=None, what=""):
    """One ops.gemm launch of configuration ``c`` -> (C, C2 or None) as views of their sentinel buffers, sentinels checked."""
    M, N = case["M"], case["N"]
    kw, bufs = epilogue_kwargs(ops, case, c, ld, zero_residual)
    if c["scale"]:
        kw["scale"] = case["scale"]
    if c["row_scale"]:
        kw["row_scale"] = case["row_scale"]
    if c["act_n0"]:
        kw["act_n0"] = ec.act_n0_of(N)
    ops.gemm(case["a"], case["lin"], accumulate=c["accumulate"], tile=tile, split_k=split_k, layout=layout, conv=conv, **kw)
    for k, b in bufs.items():
        assert_sentinels(b, M, N, f"{what} {k}")
    return bufs["C"][:M, :N], (bufs["C2"][:M, :N] if c["c2"] else None)


def check_case(case, c, C, C2, what, prod_terms=None, fp8_scales=False):
    """Assertions 1 and 4 of the file's docstring for one result."""
    R = ec.reference(case, c, prod_terms if prod_terms is not None else case.get("prod"), fp8_scales=fp8_scales)
    kcmp.assert_elementwise(C, *R["C"], f"{what} C")
    if c["c2"]:
        kcmp.assert_elementwise(C2, *R["C2"], f"{what} C2")
    if c["aux_mode"] == "relu_gate":
        closed = case["aux"] == 0
        rows, cols = ec.corner_index(case["M"], case["N"])
        assert bool(closed[rows][:, cols].all())
        exp = ec.closed_gate_expectation(case, c)
        assert torch.equal(C[closed], exp[closed]), f"{what}: a closed gate (aux = +-0.0) must leave exactly the residual sum"
    if c["aux_mode"] in ("gelu_grad", "quick_gelu_grad"):
        # aux = +30: the factor is EXACTLY 1 in the kernels' arithmetic (the exponential underflows), aux = -30: exactly 0 for
        # gelu_new_grad_f (quick_gelu_grad_f leaves ~ -4e-21 there, which the bound above covers): those elements against the
        # reference of a plain product with 1 / 0, whose factor has no error term
        (rp, cp), (rn, cn) = ec.big_index(case["M"], case["N"])
        one = torch.zeros_like(case["aux"])
        one[rp, cp] = 1.0
        Rm = ec.reference(dict(case, aux=one), dict(c, aux_mode="mul"), prod_terms if prod_terms is not None else case.get("prod"),
                          fp8_scales=fp8_scales)["C"]
        spots = [(rp, cp)] + ([(rn, cn)] if c["aux_mode"] == "gelu_grad" else [])
        for r_, c_ in spots:
            assert abs(float(C[r_, c_]) - float(Rm[0][r_, c_])) <= float(Rm[1][r_, c_]), \
                f"{what}: at aux = {float(case['aux'][r_, c_])} got {float(C[r_, c_])}, want {float(Rm[0][r_, c_])} +- {float(Rm[1][r_, c_])}"


def tile_path(dev, name, path, M, N, K, **run):
    """check_case + 'run twice' + 'with and without C2' for one configuration on one tile-GEMM path."""
    from magma_amd import ops
    c, case = ec.BY_NAME[name], problem(dev, M, N, K)
    what = f"[{path}] {name}"
    C, C2 = run_gemm(ops, case, c, what=what, **run)
    check_case(case, c, C, C2, what)
    Cb, C2b = run_gemm(ops, case, c, what=what, **run)
    assert same_bits(C, Cb) and same_bits(C2, C2b), f"{what}: a second run gave other bits"
    if c["c2"]:
        Cn, _ = run_gemm(ops, case, dict(c, c2=False), what=what, **run)
        assert same_bits(C, Cn), f"{what}: C changes when C2 is written"


# ---------------------------------------------------------------------------------------------------------------------------
# 128x128 tile kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_tile128_wide(dev, name):
    tile_path(dev, name, "128 wide", 130, 264, 128, tile=128)


@pytest.mark.parametrize("name", ALL)
def test_tile128_per_element_tail(dev, name):
    tile_path(dev, name, "128 tail", 130, 203, 128, tile=128, ld={k: 208 for k in ("c", "r", "aux", "c2")})


# every operand with a leading dimension, in a bf16 and in an accumulating fp32 configuration
NARROW = [("cover_gelu_gate", w) for w in ("c", "r", "aux", "c2")] + [("cover_quick_quick_grad", w) for w in ("c", "r", "aux", "c2")] + \
         [("bias_quick_gelu_c2", "c2"), ("quick_gelu_grad", "aux"), ("bias_res3", "r"), ("bias", "c")]


def narrow_path(dev, name, which, path, M, N, K, tile):
    """The W = 4 walk, forced by ONE leading dimension = 4 (mod 8), gives the bits of the W = 8 walk."""
    from magma_amd import ops
    c, case = ec.BY_NAME[name], problem(dev, M, N, K)
    what = f"[{path}] {name} ld{which}"
    wide, _ = run_gemm(ops, case, c, tile=tile, what=what), None
    C, C2 = run_gemm(ops, case, c, tile=tile, ld={which: ceil8(N) + 4}, what=what)
    check_case(case, c, C, C2, what)
    assert same_bits(C, wide[0]) and same_bits(C2, wide[1]), f"{what}: narrow and wide walk differ"


@pytest.mark.parametrize("name,which", NARROW)
def test_tile128_narrow(dev, name, which):
    narrow_path(dev, name, which, "128 narrow", 130, 264, 128, 128)


# ---------------------------------------------------------------------------------------------------------------------------
# 256x256 tile kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_tile256(dev, name):
    tile_path(dev, name, "256", 300, 520, 256, tile=256)


@pytest.mark.parametrize("name", ALL)
def test_tile256_per_element_tail(dev, name):
    tile_path(dev, name, "256 tail", 300, 523, 256, tile=256, ld={k: 528 for k in ("c", "r", "aux", "c2")})


@pytest.mark.parametrize("name,which", NARROW)
def test_tile256_narrow(dev, name, which):
    narrow_path(dev, name, which, "256 narrow", 300, 520, 256, 256)


NO_LOADS = [c["name"] for c in ec.CONFIGS if c["aux_mode"] == "none" and not c["n_res"] and not c["accumulate"]]


@pytest.mark.parametrize("name", NO_LOADS)
def test_tile256_build_without_loads_equals_build_with_loads(dev, name):
    """Without aux / residual / accumulate the interior tiles run epilogue_rows_c<..., LOADS = false>; a residual of zeros sends
    the same case through the LOADS = true build.  v + 0.0 changes no bit of v but the sign of a zero: torch.equal (numerical)."""
    from magma_amd import ops
    c, case = ec.BY_NAME[name], problem(dev, 300, 520, 256)
    for tile, path in ((256, "256 loads"), (128, "128 loads")):
        a = run_gemm(ops, case, c, tile=tile, what=f"[{path}] {name}")
        b = run_gemm(ops, case, c, tile=tile, zero_residual=True, what=f"[{path}] {name} + zero residual")
        assert torch.equal(a[0], b[0]), f"[{path}] {name}: C differs between the builds"
        assert c["c2"] == (a[1] is not None) and (a[1] is None or same_bits(a[1], b[1])), f"[{path}] {name}: C2 differs between the builds"
        check_case(case, c, b[0], b[1], f"[{path}] {name} + zero residual")


# (M, N, configuration): fp32 at exactly 64 MiB without / with loads; bf16 at 64 MiB without / with loads (the training shapes'
# GELU-gradient dgrad among them); N = 8200: the last column tile (8 columns) in the (NT, edge) build
NT_CASES = [(4096, 4096, "bias_f32"), (4096, 4096, "cover_gelu_mul"), (4096, 8192, "bias_gelu_c2"), (4096, 8192, "bias_res3"),
            (4096, 8192, "gelu_grad"), (4096, 8200, "scale_bias_res1_relu_after"), (4096, 8200, "bias_quick_gelu_c2")]


@pytest.mark.parametrize("M,N,name", NT_CASES)
def test_tile256_non_temporal_stores(dev, M, N, name):
    from magma_amd import ops
    c = ec.BY_NAME[name]
    assert M * N * (4 if c["out_f32"] else 2) >= 64 << 20, "gp.nt is set from 64 MiB of output"
    case = problem(dev, M, N, 128)
    what = f"[256 nt] {name} {M}x{N}"
    C, C2 = run_gemm(ops, case, c, tile=256, what=what)
    check_case(case, c, C, C2, what)
    Cb, C2b = run_gemm(ops, case, c, tile=256, what=what)
    assert same_bits(C, Cb) and same_bits(C2, C2b), f"{what}: a second run gave other bits"


def test_release_large_operands(dev):
    """Not a check: drops the 4096-row problem the items above shared, so that the rest of the suite starts from a small heap."""
    _problem.clear()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------------
# split-K: the fix-up kernel runs the epilogue (epilogue_store4)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_splitk128_fixup(dev, name):
    tile_path(dev, name, "split-K 128", 200, 203, 1024, tile=128, split_k=4, ld={k: 208 for k in ("c", "r", "aux", "c2")})


@pytest.mark.parametrize("name", ALL)
def test_splitk256_fixup(dev, name):
    tile_path(dev, name, "split-K 256", 512, 520, 2048, tile=256, split_k=2)


def test_splitk_fixup_narrow_strides(dev):
    """ldc / ldr / ldaux / ldc2 = 4 (mod 8) in the fix-up (8-byte rows either way): same bits as with multiples of 8."""
    from magma_amd import ops
    case = problem(dev, 200, 203, 1024)
    for name in ("cover_gelu_gate", "cover_quick_quick_grad", "scale_bias_res3"):
        c = ec.BY_NAME[name]
        a = run_gemm(ops, case, c, tile=128, split_k=4, ld={k: 208 for k in ("c", "r", "aux", "c2")}, what=name)
        b = run_gemm(ops, case, c, tile=128, split_k=4, ld={k: 212 for k in ("c", "r", "aux", "c2")}, what=name)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), name


# ---------------------------------------------------------------------------------------------------------------------------
# conv3x3: the implicit-im2col A loader with the epilogues of the convolution forward and backward
# ---------------------------------------------------------------------------------------------------------------------------
CONV = ["plain", "scale_bias_relu", "scale_bias_res1_relu_after", "scale_bias_relu_res1", "gate", "gate_res1", "gate_after_res1",
        "res1", "cover_relu_gate"]


@pytest.mark.parametrize("layout", ["rm", "ft"])
@pytest.mark.parametrize("name", CONV)
def test_conv3x3_epilogues(dev, name, layout):
    from magma_amd import ops
    B, H, W, Cin, Cout = 2, 12, 10, 16, 24

    def make(case):
        g = torch.Generator(device="cpu").manual_seed(77)
        x = torch.randn(B, Cin, H, W, generator=g).to(BF16).to(dev)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5).to(BF16).to(dev)
        case["a"] = x.permute(0, 2, 3, 1).contiguous().view(B * H * W, Cin)
        case["lin"] = ops.PackedLinear(w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous(), bias=case["bias"], tiled=True, rowmajor=True)
        case["prod"] = kcmp.conv2d_terms(x, w)
    c, case = ec.BY_NAME[name], problem(dev, B * H * W, Cout, 9 * Cin, make=make)
    what = f"[conv3x3 {layout}] {name}"
    C, C2 = run_gemm(ops, case, c, conv=(H, W, Cin), layout=layout, what=what)
    check_case(case, c, C, C2, what)
    Cb, C2b = run_gemm(ops, case, c, conv=(H, W, Cin), layout=layout, what=what)
    assert same_bits(C, Cb) and same_bits(C2, C2b)


# ---------------------------------------------------------------------------------------------------------------------------
# fp8 (per-row / per-channel scales) and MX (block scales), both tile kernels
# ---------------------------------------------------------------------------------------------------------------------------
F8_SHAPE = (300, 512, 256)
# mg_gemm_fp8 always applies its row-scale argument and the weight's column scale; mg_gemm_mx_fp8 applies neither; the Python
# wrappers have no accumulate.  A configuration runs with its scale fields replaced accordingly.
F8_CONFIGS = [c["name"] for c in ec.CONFIGS if not c["accumulate"] and not c["row_scale"] and not c["scale"]] + \
             ["cover_relu_gelu_grad", "cover_gelu_gate", "cover_quick_gelu_grad", "cover_relu_mul", "cover_gelu_quick_grad", "cover_quick_gate"]


def f8_problem(dev, kind):
    from magma_amd import ops
    M, N, K = F8_SHAPE

    def make(case):
        g = torch.Generator(device="cpu").manual_seed(78)
        a = torch.randn(M, K, generator=g).to(BF16).to(dev)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF16).to(dev)
        if kind == "row":
            lin = ops.PackedLinearFP8(w, bias=case["bias"], tiled=True, rowmajor=True)
            aq, asc = ops.quantize_rows_fp8(a)
            ad, wd = aq[:, :K].view(torch.float8_e4m3fn).float(), lin.dequant()       # wd carries the column scale
            case["row_scale"] = asc
        else:
            lin = ops.PackedLinearMX(w, bias=case["bias"], tiled=True, rowmajor=True)
            aq, asc = ops.quantize_mx_fp8(a)
            ad, wd = ops.mx_dequant(aq, asc, K), lin.dequant()
        p, m = kcmp.product_terms(ad, wd)
        # K products + 2 roundings for the scales (tests/test_fp8_gpu.py: dequantised_product) and the MFMA's own named term
        case.update(lin=lin, aq=aq, asc=asc, prod=(p, m, K + 2, kcmp.f8_mfma_truncation(ad, wd)))
    return problem(dev, M, N, K, seed=1 if kind == "row" else 2, make=make)


def run_f8(ops, case, c, kind, tile, what, mx_out=None, layout="ft"):
    M, N = case["M"], case["N"]
    kw, bufs = epilogue_kwargs(ops, case, c)
    fn = ops.gemm_fp8 if kind == "row" else ops.gemm_mx_fp8
    if c["act_n0"]:
        kw["act_n0"] = ec.act_n0_of(N)
    fn(case["aq"], case["asc"], case["lin"], tile=tile, split_k=1, layout=layout, mx_out=mx_out, **kw)
    for k, b in bufs.items():
        assert_sentinels(b, M, N, f"{what} {k}")
    return bufs["C"][:M, :N], (bufs["C2"][:M, :N] if c["c2"] else None)


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("kind", ["row", "mx"])
@pytest.mark.parametrize("name", F8_CONFIGS)
def test_fp8_tile_kernels(dev, name, kind, tile):
    from magma_amd import ops
    c = dict(ec.BY_NAME[name], scale=False, row_scale=kind == "row")
    if kind == "row" and c["act_n0"]:
        c["act_n0"] = False                      # ops.gemm_fp8 has no act_n0 argument: the activation on every column
    case = f8_problem(dev, kind)
    what = f"[{'fp8' if kind == 'row' else 'mx'} {tile}] {name}"
    C, C2 = run_f8(ops, case, c, kind, tile, what)
    check_case(case, c, C, C2, what)
    Cb, C2b = run_f8(ops, case, c, kind, tile, what)
    assert same_bits(C, Cb) and same_bits(C2, C2b), f"{what}: a second run gave other bits"
    if c["c2"]:
        assert same_bits(C, run_f8(ops, case, dict(c, c2=False), kind, tile, what)[0]), f"{what}: C changes when C2 is written"


@pytest.mark.parametrize("kind", ["row", "mx"])
@pytest.mark.parametrize("name", ["bias_res1", "bias_gelu_c2", "bias_quick_gelu_c2", "cover_gelu_gate", "cover_relu_quick_grad", "gelu_grad"])
def test_fp8_mx_copy_with_residual_and_activation(dev, name, kind):
    """mg_epilogue.C8 (256x256 fp8 kernels, fragment-tiled weights, N % 32 == 0): C and C2 keep their bits, the copy is what the
    quantiser makes of C, and the copy's rows >= M keep their sentinel bytes."""
    from magma_amd import ops
    M, N, _ = F8_SHAPE
    c = dict(ec.BY_NAME[name], scale=False, row_scale=kind == "row", act_n0=False if kind == "row" else ec.BY_NAME[name]["act_n0"])
    case = f8_problem(dev, kind)
    what = f"[{'fp8' if kind == 'row' else 'mx'} 256 C8] {name}"
    C, C2 = run_f8(ops, case, c, kind, 256, what)
    q = torch.full((M + 3, ops.ceil_to(N, 128)), SENT8, dtype=torch.uint8, device=dev)
    sc = ops.mx_empty(M, N, dev)[1]
    Cq, C2q = run_f8(ops, case, c, kind, 256, what, mx_out=(q, sc))
    assert same_bits(C, Cq) and same_bits(C2, C2q), f"{what}: the outputs change when the MX copy is written"
    rq, rs = ops.quantize_mx_fp8(C.contiguous())
    assert torch.equal(q[:M, :N], rq[:, :N]) and torch.equal(ops.mx_scales_rowmajor(sc, M, N), ops.mx_scales_rowmajor(rs, M, N)), what
    assert bool((q[M:] == SENT8).all()), f"{what}: the MX copy wrote to rows >= M"
    check_case(case, c, Cq, C2q, what)


# ---------------------------------------------------------------------------------------------------------------------------
# skinny GEMVs (decode): epilogue_store4 from skinny_body
# ---------------------------------------------------------------------------------------------------------------------------
# the tile-GEMM-only fields (row_scale; accumulate and act_n0, which ops.skinny_desc does not pass) stay out
SKINNY = [c["name"] for c in ec.CONFIGS if not c["row_scale"] and not c["accumulate"] and not c["act_n0"]]
SK_K = 512


def skinny_problem(dev, M, N):
    from magma_amd import ops

    def make(case):
        g = torch.Generator(device="cpu").manual_seed(79)
        case["a"] = torch.randn(M, SK_K, generator=g).to(BF16).to(dev)
        case["w"] = (torch.randn(N, SK_K, generator=g) * SK_K ** -0.5).to(BF16).to(dev)
        case["lin"] = ops.PackedLinear(case["w"], bias=case["bias"])
        p, m = kcmp.product_terms(case["a"], case["w"])
        case["prod"] = (p, m, SK_K)
    return problem(dev, M, N, SK_K, seed=3, make=make)


def skinny_kwargs(ops, case, c):
    kw, bufs = epilogue_kwargs(ops, case, c, ld={k: 208 for k in ("c", "r", "aux", "c2")} if case["N"] <= 208 else None)
    if c["scale"]:
        kw["scale"] = case["scale"]
    return kw, bufs


def run_skinny(ops, case, c, what):
    M, N = case["M"], case["N"]
    kw, bufs = skinny_kwargs(ops, case, c)
    out = kw.pop("out")
    ops.gemm_skinny(case["a"], case["lin"], out, **kw)
    for k, b in bufs.items():
        assert_sentinels(b, M, N, f"{what} {k}")
    return bufs["C"][:M, :N], (bufs["C2"][:M, :N] if c["c2"] else None)


@pytest.mark.parametrize("N", [208, 203])
@pytest.mark.parametrize("M", [1, 16])
@pytest.mark.parametrize("name", SKINNY)
def test_skinny(dev, name, M, N):
    """aux and C2 reach a GEMV through ops.skinny_desc's pass-through keywords: the general path of epilogue_store4."""
    from magma_amd import ops
    c, case = ec.BY_NAME[name], skinny_problem(dev, M, N)
    what = f"[skinny] {name} M={M} N={N}"
    C, C2 = run_skinny(ops, case, c, what)
    check_case(case, c, C, C2, what)
    Cb, C2b = run_skinny(ops, case, c, what)
    assert same_bits(C, Cb) and same_bits(C2, C2b), f"{what}: a second run gave other bits"
    if c["c2"]:
        assert same_bits(C, run_skinny(ops, case, dict(c, c2=False), what)[0]), f"{what}: C changes when C2 is written (fast against general path)"


@pytest.mark.parametrize("M", [1, 16])
@pytest.mark.parametrize("a_name,act_b,bias_b", [("bias", "gelu", True), ("scale_bias_res3", "quick_gelu", True), ("bias_gelu_c2", "none", False),
                                                 ("gate_res1", "relu", True)])
def test_skinny_split_n(dev, a_name, act_b, bias_b, M):
    """Two output segments in one launch: columns < 208 through ep (configuration a_name), the 203 columns after them through ep_b
    with an activation and a bias vector of their own (the last quad of ep_b holds 3 columns)."""
    from magma_amd import ops
    Na, Nb = 208, 203
    ca = ec.BY_NAME[a_name]
    cb = dict(ec.BY_NAME["plain"], bias=bias_b, act=act_b)
    case_a, g = ec.make_case(M, Na, SK_K, seed=4, device=dev, with_product=False), torch.Generator(device="cpu").manual_seed(80)
    case_b = ec.make_case(M, Nb, SK_K, seed=5, device=dev, with_product=False)
    x = torch.randn(M, SK_K, generator=g).to(BF16).to(dev)
    w = (torch.randn(Na + Nb, SK_K, generator=g) * SK_K ** -0.5).to(BF16).to(dev)
    lin = ops.PackedLinear(w, bias=case_a["bias"])
    kw, bufs = skinny_kwargs(ops, case_a, ca)
    out_a = kw.pop("out")
    bbuf, out_b = padded(torch.full((M, Nb), SENT, dtype=BF16, device=dev), 208, 3)
    ops.gemm_skinny(x, lin, out_a, split=(Na, out_b, codes(ops, cb)[0], case_b["bias"] if bias_b else None), **kw)
    what = f"[skinny split_n] {a_name} | {act_b} M={M}"
    for k, b in bufs.items():
        assert_sentinels(b, M, Na, f"{what} {k}")
    assert_sentinels(bbuf, M, Nb, f"{what} segment b")
    pa, ma = kcmp.product_terms(x, w[:Na])
    pb, mb = kcmp.product_terms(x, w[Na:])
    check_case(case_a, ca, bufs["C"][:M, :Na], bufs["C2"][:M, :Na] if ca["c2"] else None, what + " segment a", prod_terms=(pa, ma, SK_K))
    check_case(case_b, cb, out_b, None, what + " segment b", prod_terms=(pb, mb, SK_K))


DECODE = ["bias", "bias_f32", "bias_relu", "bias_res2", "bias_res3", "scale_bias_res1", "scale_bias_res3"]       # engine.py:884-984


@pytest.mark.parametrize("a_name,b_name", [("bias_res2", "bias_relu"), ("scale_bias_res3", "bias_gelu"), ("bias_res3", "scale_bias_res1"),
                                           ("bias_f32", "cover_gelu_gate")])
def test_skinny2_pair(dev, a_name, b_name):
    """out_proj || adapter-down in one launch (skinny2_kernel<4, 1, 1> at K = 512), N = 203 and 208, M = 8."""
    from magma_amd import ops
    M = 8
    cases, runs = [], []
    for i, (name, N) in enumerate(((a_name, 203), (b_name, 208))):
        c = ec.BY_NAME[name]
        case = ec.make_case(M, N, SK_K, seed=6 + i, device=dev)
        lin = ops.PackedLinear(case["w"], bias=case["bias"])
        kw, bufs = skinny_kwargs(ops, case, c)
        cases.append((c, case, bufs, N))
        runs.append((case["a"], lin, kw.pop("out"), kw))
    ops.gemm_skinny2(*runs)
    for c, case, bufs, N in cases:
        what = f"[skinny2] {c['name']} N={N}"
        for k, b in bufs.items():
            assert_sentinels(b, M, N, f"{what} {k}")
        check_case(case, c, bufs["C"][:M, :N], bufs["C2"][:M, :N] if c["c2"] else None, what)


@pytest.mark.parametrize("name", DECODE)
def test_attention_gemv_colaunch(dev, name):
    """decode_attn_gemv_kernel<4>: the GEMV half runs skinny_body with the configurations the decode step issues; the attention
    half writes what the stand-alone fused decode attention writes."""
    from magma_amd import ops
    from oracle.model import rotary_tables
    B, H, Smax, ctx, N = 3, 2, 192, 57, 203
    d = H * 256
    g = torch.Generator(device="cpu").manual_seed(81)
    kc0 = (torch.randn(B, H, Smax, 256, generator=g) * 0.5).to(BF16).to(dev)
    vc0 = torch.randn(B, H, Smax, 256, generator=g).to(BF16).to(dev)
    qkv = (torch.randn(B, 3 * d, generator=g) * 0.5).to(BF16).to(dev)
    sin_t, cos_t = (t.to(dev).contiguous() for t in rotary_tables(64, Smax))
    d_pos = torch.tensor([ctx - 1], dtype=torch.int32, device=dev)
    c = ec.BY_NAME[name]
    case = ec.make_case(B, N, SK_K, seed=8, device=dev)
    lin = ops.PackedLinear(case["w"], bias=case["bias"])
    kw, bufs = skinny_kwargs(ops, case, c)
    out = kw.pop("out")
    kc, vc, att = kc0.clone(), vc0.clone(), torch.empty(B, d, dtype=BF16, device=dev)
    ops.decode_attn_gemv(qkv, kc, vc, att, B, H, d_pos, 64, sin_t, cos_t, (case["a"], lin, out, kw))
    what = f"[attention+GEMV] {name}"
    assert_sentinels(bufs["C"], B, N, what)
    check_case(case, c, bufs["C"][:B, :N], None, what)
    kc2, vc2, att2 = kc0.clone(), vc0.clone(), torch.empty(B, d, dtype=BF16, device=dev)
    ops.attn_decode_fused(qkv, kc2, vc2, att2, B, H, d_pos, 64, sin_t, cos_t)
    assert torch.equal(att, att2) and torch.equal(kc, kc2) and torch.equal(vc, vc2), f"{what}: the attention half differs from the stand-alone launch"
