"""Operands past 4 GiB: every op below runs with exactly ONE operand inside a 17-GiB arena (tests/far_operands.py), placed so
that some of its rows start past 2^32 bytes / 2^31 elements from its base pointer, and is held to

  (a) the fp64 reference and the per-element bound of the op's own test (tests/kernel_compare.py; copies are bit-exact),
  (b) bit-for-bit equality with the same call on a tight, low-address copy of the same values -- every op here is deterministic
      except the atomic column sums (``colsum`` without ``deterministic``, ``transpose_colsum``), which get (a) only,
  (c) an arena that is 0xFF everywhere outside the operand afterwards (no store went to an alias).

A kernel that wraps a 32-bit offset reads poison (NaN) or another row and fails (a) and (b); tests/test_far_operands_cpu.py shows
that it cannot leave the arena.  Operands the library cannot address are refused: MagmaHipError, nothing launched."""
import pytest
import torch

import far_operands as far
import kernel_compare as kcmp

pytestmark = pytest.mark.gpu

BF16, F32, U8, I64 = torch.bfloat16, torch.float32, torch.uint8, torch.int64
EPS = 1e-5


@pytest.fixture(scope="module")
def arena(dev):
    """The only large allocation alive; an out-of-memory error here fails the tests."""
    buf = torch.empty(far.ARENA_BYTES, dtype=U8, device=dev)
    yield buf
    del buf
    torch.cuda.empty_cache()


def rnd(*shape, scale=1.0, seed=0, dtype=BF16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def bits(t):
    return far.as_ints(t.contiguous())


def place(arena, name, data=None, fresh=True):
    """Poison the arena (unless ``fresh`` is False: a second operand of the same call) and return (view, writable region) of
    case ``name``; ``data`` (if any) is copied into the view."""
    case = far.CASES[name]
    if fresh:
        far.poison(arena)
    lay = case.layout()
    region, _ = far.far_view(arena, case.dtype, lay.shape, lay.strides, case.skew)
    view = region[..., : case.shape[-1]] if case.pad_cols else region
    assert tuple(view.shape) == case.shape
    if data is not None:
        assert tuple(data.shape) == case.shape and data.dtype == case.dtype
        view.copy_(data)
    return view, region


def finish(arena, region, what):
    """(c): with the operand's own region wiped, nothing else of the arena may have changed."""
    torch.cuda.synchronize()
    far.wipe(region)
    far.assert_arena_poison(arena, what)


def assert_same_bits(far_result, near_result, what):
    assert torch.equal(bits(far_result), bits(near_result)), f"{what}: the far operand and its near copy give different bits"


# ---------------------------------------------------------------------------------------------------------------------------
# tile GEMMs
# ---------------------------------------------------------------------------------------------------------------------------
M, K, N = far.GEMM_M, far.GEMM_K, far.GEMM_N
TILES = (128, 256)
SPLITS = (1, 2)


@pytest.fixture(scope="module")
def gemm_operands(dev):
    """Shared by the GEMM cases and left unchanged: A [M, K], W [N, K], bias, and the fp64 product terms."""
    a = rnd(M, K, seed=1).to(dev)
    w = rnd(N, K, scale=K ** -0.5, seed=2).to(dev)
    bias = rnd(N, seed=3, dtype=F32).to(dev)
    p, m = kcmp.product_terms(a, w)
    return {"a": a, "w": w, "bias": bias, "prod": (p, m, K)}


def check_c(out, ref, what):
    kcmp.assert_elementwise(out, ref[0], ref[1], what)


@pytest.mark.parametrize("layout", ["rm", "ft"])
@pytest.mark.parametrize("split_k", SPLITS)
@pytest.mark.parametrize("tile", TILES)
def test_gemm_far_a(dev, arena, gemm_operands, tile, split_k, layout):
    from magma_amd import ops
    g = gemm_operands
    what = f"gemm far A tile={tile} split_k={split_k} {layout}"
    lin = ops.PackedLinear(g["w"], bias=g["bias"], tiled=True, rowmajor=True)
    a_far, region = place(arena, "gemm_a", g["a"])
    kw = dict(tile=tile, split_k=split_k, layout=layout)
    out = ops.gemm(a_far, lin, **kw)
    check_c(out, kcmp.epilogue_reference(g["prod"], bias=g["bias"])["C"], what)
    assert_same_bits(out, ops.gemm(g["a"], lin, **kw), what)
    assert torch.equal(bits(a_far), bits(g["a"])), f"{what}: A was written"
    finish(arena, region, what)


@pytest.mark.parametrize("split_k", SPLITS)
@pytest.mark.parametrize("tile", TILES)
def test_gemm_far_w(dev, arena, gemm_operands, tile, split_k):
    """The far operand as a row-major RawWeight [600, 256] (the transposed activations of the weight-gradient GEMMs): the roles
    of the two shared matrices swap, out[n, m] = W[n] . A[m]."""
    from magma_amd import ops
    g = gemm_operands
    what = f"gemm far row-major W tile={tile} split_k={split_k}"
    x = g["w"]                                   # [264, 256] as the A operand
    w_far, region = place(arena, "gemm_w", g["a"])
    kw = dict(tile=tile, split_k=split_k, layout="rm", use_bias=False)
    out = ops.gemm(x, ops.RawWeight(w_far), **kw)
    p, m, _ = g["prod"]
    check_c(out, kcmp.epilogue_reference((p.t(), m.t(), K))["C"], what)
    assert_same_bits(out, ops.gemm(x, ops.RawWeight(g["a"]), **kw), what)
    finish(arena, region, what)


@pytest.mark.parametrize("layout", ["rm", "ft"])
@pytest.mark.parametrize("split_k", SPLITS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", ["gemm_out_bf16", "gemm_out_f32"])
def test_gemm_far_output(dev, arena, gemm_operands, name, tile, split_k, layout):
    from magma_amd import ops
    g = gemm_operands
    case = far.CASES[name]
    rows = case.shape[0]
    what = f"{case.op} tile={tile} split_k={split_k} {layout}"
    lin = ops.PackedLinear(g["w"], bias=g["bias"], tiled=True, rowmajor=True)
    out_far, region = place(arena, name)
    a = g["a"][:rows]
    kw = dict(tile=tile, split_k=split_k, layout=layout)
    assert ops.gemm(a, lin, out=out_far, **kw) is out_far
    p, m, _ = g["prod"]
    check_c(out_far, kcmp.epilogue_reference((p[:rows], m[:rows], K), bias=g["bias"], out_dtype=case.dtype)["C"], what)
    assert_same_bits(out_far, ops.gemm(a, lin, out_dtype=case.dtype, **kw), what)
    finish(arena, region, what)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", ["gemm_residual", "gemm_aux", "gemm_out2"])
def test_gemm_far_epilogue_operand(dev, arena, gemm_operands, name, tile):
    """One epilogue per operand (tests/test_gemm_epilogue_matrix_gpu.py owns the rest): a far residual (ldr), a far aux factor
    (MG_AUX_MUL, ldaux) and a far second output (C2, ldc2)."""
    from magma_amd import ops
    g = gemm_operands
    what = f"{far.CASES[name].op} tile={tile}"
    lin = ops.PackedLinear(g["w"], bias=g["bias"])
    extra = rnd(M, N, seed=7).to(dev)
    kw = dict(tile=tile, split_k=1)
    if name == "gemm_residual":
        view, region = place(arena, name, extra)
        out = ops.gemm(g["a"], lin, residuals=(view,), **kw)
        ref = kcmp.epilogue_reference(g["prod"], bias=g["bias"], residuals=(extra,))
        near = ops.gemm(g["a"], lin, residuals=(extra,), **kw)
    elif name == "gemm_aux":
        view, region = place(arena, name, extra)
        out = ops.gemm(g["a"], lin, aux=view, aux_mode=ops.MG_AUX_MUL, **kw)
        ref = kcmp.epilogue_reference(g["prod"], bias=g["bias"], aux=extra, aux_mode="mul")
        near = ops.gemm(g["a"], lin, aux=extra, aux_mode=ops.MG_AUX_MUL, **kw)
    else:
        view, region = place(arena, name)
        out = ops.gemm(g["a"], lin, act=ops.MG_ACT_GELU_NEW, out2=view, **kw)
        ref = kcmp.epilogue_reference(g["prod"], bias=g["bias"], act="gelu")
        near2 = torch.empty(M, N, dtype=BF16, device=dev)
        near = ops.gemm(g["a"], lin, act=ops.MG_ACT_GELU_NEW, out2=near2, **kw)
        check_c(view, ref["C2"], what + " (C2)")
        assert_same_bits(view, near2, what + " (C2)")
    check_c(out, ref["C"], what)
    assert_same_bits(out, near, what)
    if name != "gemm_out2":
        assert torch.equal(bits(view), bits(extra)), f"{what}: the operand was written"
    finish(arena, region, what)


def test_gemm256_refuses_strides_its_loaders_cannot_hold(dev, arena, gemm_operands):
    """256 rows of A, or of a row-major W, must span less than 2^32 bytes on the 256x256 kernel (its loaders add a 32-bit
    per-lane byte offset to the workgroup's 64-bit row origin).  A forced tile is refused, naming the limit; without a forced
    tile the same operand goes to the 128x128 kernel and is computed correctly."""
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    g = gemm_operands
    far.poison(arena)
    rows, ld = 264, far.GEMM256_LD_LIMIT
    wide, _ = far.far_view(arena, BF16, (rows, K), (ld, 1))
    lin = ops.PackedLinear(g["w"], bias=g["bias"], tiled=True, rowmajor=True)
    for split_k in SPLITS:
        with pytest.raises(MagmaHipError, match="32-bit byte offsets of the 256x256 tile loaders"):
            ops.gemm(wide, lin, tile=256, split_k=split_k)
        with pytest.raises(MagmaHipError, match="32-bit byte offsets of the 256x256 tile loaders"):
            ops.gemm(g["a"], ops.RawWeight(wide), tile=256, split_k=split_k, layout="rm", use_bias=False)
    torch.cuda.synchronize()
    far.assert_arena_poison(arena, "refused 256x256 GEMMs")
    # one row stride below the limit is taken
    ok, _ = far.far_view(arena, BF16, (rows, K), (ld - 8, 1))
    ok.copy_(g["a"][:rows])
    p, m, _ = g["prod"]
    ref = kcmp.epilogue_reference((p[:rows], m[:rows], K), bias=g["bias"])["C"]
    a_near = g["a"][:rows].contiguous()
    out = ops.gemm(ok, lin, tile=256, split_k=1)
    check_c(out, ref, "gemm tile=256 at lda = 2^23 - 8")
    assert_same_bits(out, ops.gemm(a_near, lin, tile=256, split_k=1), "gemm tile=256 at lda = 2^23 - 8")
    finish(arena, ok, "gemm tile=256 at lda = 2^23 - 8")
    # at the limit, tile 0 and tile 128 run the 128x128 kernel
    wide.copy_(a_near)
    for tile in (0, 128):
        out = ops.gemm(wide, lin, tile=tile, split_k=1)
        check_c(out, ref, f"gemm tile={tile} at lda = 2^23")
        assert_same_bits(out, ops.gemm(a_near, lin, tile=tile, split_k=1), f"gemm tile={tile} at lda = 2^23")
    finish(arena, wide, "gemm tile 0 / 128 at lda = 2^23")


def test_mx_output_copy_is_refused_past_the_256_row_limit(dev, arena, gemm_operands):
    """The MX output copy (mg_epilogue.C8) is written by the 256x256 fp8 kernel only: with an A whose 256 rows span 2^32 bytes
    there is no kernel to fall back to, so both fp8 GEMMs refuse it, whatever the tile hint, naming the limit.  Nothing is
    launched: the arena and the copy stay as they were."""
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    g = gemm_operands
    far.poison(arena)
    rows, ld = 264, 2 * far.GEMM256_LD_LIMIT                        # bytes: 2^23 pairs of fp8 values
    N8 = 256                                                        # the copy needs N % 32 == 0
    wide, _ = far.far_view(arena, U8, (rows, K), (ld, 1))
    w = g["w"][:N8]
    for form in ("rows", "mx"):
        if form == "rows":
            lin = ops.PackedLinearFP8(w)
            _, asc = ops.quantize_rows_fp8(g["a"][:rows])
            run = lambda **kw: ops.gemm_fp8(wide, asc, lin, **kw)
        else:
            lin = ops.PackedLinearMX(w)
            _, asc = ops.quantize_mx_fp8(g["a"][:rows])
            run = lambda **kw: ops.gemm_mx_fp8(wide, asc, lin, **kw)
        for tile in (0, 256):
            q, sc = ops.mx_empty(rows, N8, dev)
            q.fill_(0xA5)
            sc0 = sc.clone()
            with pytest.raises(MagmaHipError, match="32-bit byte offsets of the 256x256 tile loaders.*MX output copy"):
                run(tile=tile, mx_out=(q, sc))
            torch.cuda.synchronize()
            assert bool((q == 0xA5).all()) and torch.equal(sc, sc0), "a refused launch wrote the MX copy"
        with pytest.raises(MagmaHipError, match="32-bit byte offsets of the 256x256 tile loaders"):
            run(tile=256)
    far.assert_arena_poison(arena, "refused fp8 GEMMs")


# ---------------------------------------------------------------------------------------------------------------------------
# skinny GEMV
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["skinny_x", "skinny_out"])
def test_gemm_skinny_far(dev, arena, name):
    from magma_amd import ops
    Ms, Ks = 16, 1024
    x = rnd(Ms, Ks, seed=11).to(dev)
    w = rnd(N, Ks, scale=Ks ** -0.5, seed=12).to(dev)
    bias = rnd(N, seed=13, dtype=F32).to(dev)
    lin = ops.PackedLinear(w, bias=bias)
    what = far.CASES[name].op
    near = ops.gemm_skinny(x, lin)
    if name == "skinny_x":
        view, region = place(arena, name, x)
        out = ops.gemm_skinny(view, lin)
    else:
        out, region = place(arena, name)
        assert ops.gemm_skinny(x, lin, out=out) is out
    kcmp.assert_linear(out, what, x, w, bias=bias)
    assert_same_bits(out, near, what)
    finish(arena, region, what)


# ---------------------------------------------------------------------------------------------------------------------------
# row and movement kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["layernorm_x", "layernorm_out"])
def test_layernorm_far(dev, arena, name):
    from magma_amd import ops
    rows, d = far.CASES[name].shape
    x = (rnd(rows, d, seed=21).float() + 0.5).to(BF16).to(dev)
    g = (rnd(d, seed=22, dtype=F32) * 0.1 + 1).to(dev)
    b = (rnd(d, seed=23, dtype=F32) * 0.1 + 0.25).to(dev)
    what = far.CASES[name].op
    near = ops.layernorm(x, g, b, EPS)
    if name == "layernorm_x":
        view, region = place(arena, name, x)
        out = ops.layernorm(view, g, b, EPS)
    else:
        out, region = place(arena, name)
        assert ops.layernorm(x, g, b, EPS, out=out) is out
    T = kcmp.layernorm_terms(x, g, b, EPS)
    kcmp.assert_elementwise(out, T["ref"], kcmp.layernorm_bound(T, d), what)
    assert_same_bits(out, near, what)
    finish(arena, region, what)


@pytest.mark.parametrize("name", ["layernorm_bwd_x", "layernorm_bwd_dy"])
def test_layernorm_bwd_far(dev, arena, name):
    from magma_amd import ops
    rows, d = far.CASES[name].shape
    x = (rnd(rows, d, seed=31).float() + 0.5).to(BF16).to(dev)
    dy = rnd(rows, d, seed=32).to(dev)
    g = (rnd(d, seed=33, dtype=F32) * 0.1 + 1).to(dev)
    what = far.CASES[name].op
    near_dx, near_xh = ops.layernorm_bwd(dy, x, g, EPS, want_xhat=True)
    view, region = place(arena, name, x if name == "layernorm_bwd_x" else dy)
    dx, xh = ops.layernorm_bwd(dy, view, g, EPS, want_xhat=True) if name == "layernorm_bwd_x" else ops.layernorm_bwd(view, x, g, EPS, want_xhat=True)
    ref = kcmp.layernorm_bwd_reference(dy, x, g, EPS)
    kcmp.assert_elementwise(dx, *ref["dx"], what + " dx")
    kcmp.assert_elementwise(xh, *ref["xhat"], what + " xhat")
    assert_same_bits(dx, near_dx, what + " dx")
    assert_same_bits(xh, near_xh, what + " xhat")
    finish(arena, region, what)


@pytest.fixture(scope="module")
def logits_case(dev):
    R, V = far.CASES["ce_logits"].shape
    logits = rnd(R, V, scale=3.0, seed=41, dtype=F32).to(dev)
    targets = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(42)).to(dev)
    targets[5] = -100
    return logits, targets, kcmp.cross_entropy_reference(logits, targets)


def test_cross_entropy_far_logits(dev, arena, logits_case):
    from magma_amd import ops
    logits, targets, ref = logits_case
    R, V = logits.shape
    what = "cross_entropy, far fp32 logits"
    view, region = place(arena, "ce_logits", logits)
    mean, rows = ops.cross_entropy(view, targets)
    kcmp.assert_elementwise(rows, *ref["rows"], what + " rows")
    kcmp.assert_elementwise(mean.reshape(1), *ref["mean"], what + " mean")
    near_mean, near_rows = ops.cross_entropy(logits, targets)
    assert_same_bits(rows, near_rows, what + " rows")
    assert_same_bits(mean.reshape(1), near_mean.reshape(1), what + " mean")
    ld_out = V + 3
    loss, dl = ops.cross_entropy_fwd_bwd(view, targets, ld_out)
    kcmp.assert_elementwise(dl[:, :V], *ref["dlogits"], what + " dlogits")
    assert bool((dl[:, V:] == 0).all())
    assert_same_bits(dl, ops.cross_entropy_fwd_bwd(logits, targets, ld_out)[1], what + " dlogits")
    assert torch.equal(bits(view), bits(logits)), f"{what}: the logits were written"
    finish(arena, region, what)


def test_argmax_far_logits(dev, arena, logits_case):
    from magma_amd import ops
    logits = logits_case[0]
    view, region = place(arena, "ce_logits", logits)
    got = ops.argmax(view)
    assert torch.equal(got, logits.double().argmax(-1)), "argmax, far fp32 logits"          # random fp32 rows: no ties
    assert torch.equal(got, ops.argmax(logits))
    finish(arena, region, "argmax, far fp32 logits")


def test_colsum_far(dev, arena):
    from magma_amd import ops
    rows, d = far.CASES["colsum_x"].shape
    x = rnd(rows, d, seed=51).to(dev)
    view, region = place(arena, "colsum_x", x)
    s, mag = x.double().sum(0), x.double().abs().sum(0)
    out = ops.colsum(view, torch.zeros(d, dtype=F32, device=dev))
    kcmp.assert_elementwise(out, s, kcmp.rounded(s, kcmp.gamma(rows + 8) * mag, F32), "colsum (atomic), far x")
    det = ops.colsum(view, torch.zeros(d, dtype=F32, device=dev), deterministic=True)
    kcmp.assert_elementwise(det, s, kcmp.rounded(s, kcmp.gamma(rows + 9) * mag, F32), "colsum (deterministic), far x")
    assert_same_bits(det, ops.colsum(x, torch.zeros(d, dtype=F32, device=dev), deterministic=True), "colsum (deterministic), far x")
    finish(arena, region, "colsum, far x")


def test_transpose_far_input(dev, arena):
    from magma_amd import ops
    rows, d = far.CASES["transpose_in"].shape
    x = rnd(rows, d, seed=61).to(dev)
    view, region = place(arena, "transpose_in", x)
    xt = ops.transpose(view)
    assert torch.equal(bits(xt[:, :rows]), bits(x.t())) and bool((xt[:, rows:] == 0).all()), "transpose, far input"
    acc = torch.full((d,), 0.5, dtype=F32, device=dev)
    xt2 = ops.transpose_colsum(view, acc)
    assert torch.equal(bits(xt2), bits(xt)), "transpose_colsum, far input: the transpose"
    s, mag = 0.5 + x.double().sum(0), 0.5 + x.double().abs().sum(0)
    kcmp.assert_elementwise(acc, s, kcmp.rounded(s, kcmp.gamma(rows + 9) * mag, F32), "transpose_colsum, far input: the sums")
    finish(arena, region, "transpose / transpose_colsum, far input")


def test_transpose_far_output(dev, arena):
    """Input [37, 600] -> output [600, 40] at a far row stride; columns 37 .. 39 are the documented zero padding."""
    from magma_amd import ops
    case = far.CASES["transpose_out"]
    C, R = case.shape
    x = rnd(R, C, seed=62).to(dev)
    out, region = place(arena, "transpose_out")
    assert ops.transpose(x, out=region) is region
    assert torch.equal(bits(out), bits(x.t())), "transpose, far output"
    assert bool((region[:, R:] == 0).all()), "transpose, far output: the padding columns"
    assert_same_bits(region, ops.transpose(x), "transpose, far output")
    finish(arena, region, "transpose, far output")


def test_transpose_colsum_far_output(dev, arena):
    """The same output view through transpose_colsum: the transpose bit for bit, the column sums under test_colsum's bound."""
    from magma_amd import ops
    case = far.CASES["transpose_out"]
    C, R = case.shape
    x = rnd(R, C, seed=63).to(dev)
    out, region = place(arena, "transpose_out")
    acc = torch.full((C,), 0.5, dtype=F32, device=dev)
    assert ops.transpose_colsum(x, acc, out=region) is region
    assert torch.equal(bits(out), bits(x.t())), "transpose_colsum, far output"
    assert bool((region[:, R:] == 0).all()), "transpose_colsum, far output: the padding columns"
    assert_same_bits(region, ops.transpose(x), "transpose_colsum, far output")
    s_, mag = 0.5 + x.double().sum(0), 0.5 + x.double().abs().sum(0)
    kcmp.assert_elementwise(acc, s_, kcmp.rounded(s_, kcmp.gamma(R + 9) * mag, F32), "transpose_colsum, far output: the sums")
    finish(arena, region, "transpose_colsum, far output")


@pytest.mark.parametrize("name", ["gelu_x", "gelu_out"])
def test_gelu_erf_far(dev, arena, name):
    from magma_amd import ops
    rows, d = far.CASES[name].shape
    x = rnd(rows, d, scale=2.0, seed=71).to(dev)
    what = far.CASES[name].op
    near = ops.gelu_erf(x)
    if name == "gelu_x":
        view, region = place(arena, name, x)
        out = ops.gelu_erf(view)
    else:
        out, region = place(arena, name)
        assert ops.gelu_erf(x, out=out) is out
    ge, ge_err, _, _ = kcmp.gelu_erf_terms(x)
    kcmp.assert_elementwise(out, ge, kcmp.rounded(ge, ge_err, BF16), what)
    assert_same_bits(out, near, what)
    finish(arena, region, what)


def test_scale_rows_acc_far_src(dev, arena):
    """dst += src * row_scale[r] in fp32: one product and one addition per element."""
    from magma_amd import ops
    rows, d = far.CASES["scale_rows_src"].shape
    src = rnd(rows, d, seed=81, dtype=F32).to(dev)
    scale = rnd(rows, seed=82, dtype=F32).to(dev)
    start = rnd(rows, d, seed=83, dtype=F32).to(dev)
    view, region = place(arena, "scale_rows_src", src)
    dst, near = start.clone(), start.clone()
    ops.scale_rows_acc(dst, view, scale)
    ops.scale_rows_acc(near, src, scale)
    prod = src.double() * scale.double()[:, None]
    ref = start.double() + prod
    kcmp.assert_elementwise(dst, ref, kcmp.rounded(ref, kcmp.gamma(2) * (start.double().abs() + prod.abs()), F32), "scale_rows_acc, far src")
    assert_same_bits(dst, near, "scale_rows_acc, far src")
    finish(arena, region, "scale_rows_acc, far src")


def test_quantize_rows_fp8_far_x(dev, arena):
    """Reference and comparison of tests/test_fp8_gpu.py::test_quantize_rows: the scales and the e4m3 values equal ref_quant's."""
    from magma_amd import ops
    from test_fp8_gpu import ref_quant
    rows, d = far.CASES["quantize_rows_x"].shape
    x = (rnd(rows, d, seed=91).float() * torch.logspace(-3, 2, rows)[:, None]).to(BF16).to(dev)
    view, region = place(arena, "quantize_rows_x", x)
    q, sc = ops.quantize_rows_fp8(view)
    rq, rs = ref_quant(x)
    assert torch.equal(sc, rs), "quantize_rows_fp8, far x: scales"
    assert q.shape[1] % 128 == 0 and bool((q[:, d:] == 0).all())
    assert torch.equal(q[:, :d].view(torch.float8_e4m3fn).float(), rq.float()), "quantize_rows_fp8, far x: codes"
    nq, nsc = ops.quantize_rows_fp8(x)
    assert_same_bits(q, nq, "quantize_rows_fp8, far x: codes")
    assert_same_bits(sc, nsc, "quantize_rows_fp8, far x: scales")
    assert torch.equal(bits(view), bits(x)), "quantize_rows_fp8, far x: x was written"
    finish(arena, region, "quantize_rows_fp8, far x")


def test_token_logprobs_far_logits(dev, arena, logits_case):
    """The chosen token's log-probability and the three most probable tokens per row, bound and comparator of
    tests/test_logprobs_gpu.py."""
    from magma_amd import ops
    from test_logprobs_gpu import _within
    logits, targets, _ = logits_case
    R, V = logits.shape
    tok = targets.clamp(min=0)
    view, region = place(arena, "ce_logits", logits)

    def run(x):
        lp = torch.full((R, 1), float("nan"), device=dev)
        tid = torch.full((R, 1, 3), -7, dtype=torch.int32, device=dev)
        tl = torch.full((R, 1, 3), float("nan"), device=dev)
        ops.token_logprobs(x, tok, lp, tid, tl)
        return lp, tid, tl

    lp, tid, tl = run(view)
    ref = torch.log_softmax(logits.double(), -1)
    top = ref.topk(3, -1)
    assert torch.equal(tid[:, 0].long(), top.indices), "token_logprobs, far logits: the ranked ids"
    _within(lp[:, 0].cpu(), ref.gather(1, tok[:, None])[:, 0].cpu(), V, "token_logprobs, far logits: lp")
    _within(tl[:, 0].cpu(), top.values.cpu(), V, "token_logprobs, far logits: top_lp")
    for got, near in zip((lp, tid, tl), run(logits)):
        assert_same_bits(got, near, "token_logprobs, far logits")
    finish(arena, region, "token_logprobs, far logits")


def test_rotary_split_far_qkv(dev, arena):
    """One sequence of 600 positions, one head: q, k turned (rotary_reference), v copied, from qkv rows at a far ld_qkv."""
    from magma_amd import ops
    from oracle.model import rotary_tables
    S, W3 = far.CASES["rotary_qkv"].shape
    Smax = 640
    x = rnd(S, W3, scale=0.5, seed=131).to(dev)
    sin_t, cos_t = rotary_tables(64, Smax)
    sin_t, cos_t = sin_t.to(dev).contiguous(), cos_t.to(dev).contiguous()
    view, region = place(arena, "rotary_qkv", x)

    def run(qkv):
        q = torch.full((1, 1, S, 256), float("nan"), dtype=BF16, device=dev)
        kc = torch.full((1, 1, Smax, 256), float("nan"), dtype=BF16, device=dev)
        vc = torch.full((1, 1, Smax, 256), float("nan"), dtype=BF16, device=dev)
        ops.rotary_split(qkv, 1, S, 1, 64, sin_t, cos_t, q, kc, vc, pos0=0)
        return q, kc, vc

    q, kc, vc = run(view)
    xd = x.view(1, S, 3, 1, 256).permute(2, 0, 3, 1, 4)               # [3, B, H, S, 256]
    for got, src, name in ((q, xd[0], "q"), (kc[:, :, :S], xd[1], "k")):
        kcmp.assert_elementwise(got, *kcmp.rotary_reference(src, sin_t[:S], cos_t[:S], 64), f"rotary_split, far qkv: {name}")
    assert torch.equal(bits(vc[:, :, :S]), bits(xd[2])), "rotary_split, far qkv: v"
    assert bool(torch.isnan(kc[:, :, S:].float()).all()) and bool(torch.isnan(vc[:, :, S:].float()).all())
    for got, near in zip((q, kc, vc), run(x)):
        assert_same_bits(got, near, "rotary_split, far qkv")
    assert torch.equal(bits(view), bits(x)), "rotary_split, far qkv: qkv was written"
    finish(arena, region, "rotary_split, far qkv")


def test_head_transpose_far_src(dev, arena):
    """out[b, h, t, d, i] = src[b, 32 t + i, h, d], zero padded to whole 32-position tiles: a copy, bit for bit."""
    from magma_amd import ops
    S, D = far.CASES["head_transpose_src"].shape
    x = rnd(S, D, seed=101).to(dev)
    view, region = place(arena, "head_transpose_src", x)
    ss = view.stride(0)
    out = ops.head_transpose(view, 1, 1, S, S * ss, ss, D)
    Sp = (S + 31) // 32 * 32
    padded = torch.zeros(Sp, D, dtype=BF16, device=dev)
    padded[:S] = x
    want = padded.view(Sp // 32, 32, D).permute(0, 2, 1).reshape(1, 1, Sp // 32, D, 32)
    assert torch.equal(bits(out), bits(want)), "head_transpose, far src"
    assert_same_bits(out, ops.head_transpose(x, 1, 1, S, S * D, D, D), "head_transpose, far src")
    finish(arena, region, "head_transpose, far src")


def test_embedding_far_out(dev, arena):
    from magma_amd import ops
    B, T, d = far.CASES["embedding_out"].shape
    wte = rnd(50, d, seed=111).to(dev)
    ids = torch.randint(0, 50, (B, T), generator=torch.Generator().manual_seed(112)).to(dev)
    out, region = place(arena, "embedding_out")
    assert ops.embedding(ids, wte, out) is out
    assert torch.equal(bits(out), bits(wte[ids])), "embedding, far out"
    finish(arena, region, "embedding, far out")


def test_quantize_mx_fp8_far_x(dev, arena):
    """Reference and comparison of tests/test_fp8_gpu.py::test_quantize_mx: block scales and e4m3 values equal _mx_ref_quant's."""
    from magma_amd import ops
    from test_fp8_gpu import _mx_ref_quant
    rows, d = far.CASES["quantize_mx_x"].shape
    x = (rnd(rows, d, seed=92).float() * torch.logspace(-3, 2, rows)[:, None]).to(BF16).to(dev)
    x[-1, 32:64] = 0                                                # an all-zero block
    view, region = place(arena, "quantize_mx_x", x)
    q, sc = ops.quantize_mx_fp8(view)
    rq, re = _mx_ref_quant(x)
    assert torch.equal(ops.mx_scales_rowmajor(sc, rows, q.shape[1]).float(), re), "quantize_mx_fp8, far x: block scales"
    assert torch.equal(q.view(torch.float8_e4m3fn).float(), rq), "quantize_mx_fp8, far x: codes"
    nq, nsc = ops.quantize_mx_fp8(x)
    assert_same_bits(q, nq, "quantize_mx_fp8, far x: codes")
    assert_same_bits(sc, nsc, "quantize_mx_fp8, far x: block scales")
    assert torch.equal(bits(view), bits(x)), "quantize_mx_fp8, far x: x was written"
    finish(arena, region, "quantize_mx_fp8, far x")


# ---------------------------------------------------------------------------------------------------------------------------
# fp8 GEMMs with the quantised A far
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("form", ["rows", "mx"])
def test_gemm_fp8_far_a(dev, arena, gemm_operands, form, tile):
    """(b) against the near copy bit for bit, and (a) through it: tests/test_fp8_gpu.py and the epilogue matrix hold the near
    call to the fp64 reference of the dequantised operands; here the same reference is applied to the far call."""
    from magma_amd import ops
    g = gemm_operands
    what = f"gemm_{'mx_' if form == 'mx' else ''}fp8 far A tile={tile}"
    if form == "rows":
        lin = ops.PackedLinearFP8(g["w"], bias=g["bias"])
        aq, asc = ops.quantize_rows_fp8(g["a"])
        run = lambda a8: ops.gemm_fp8(a8, asc, lin, tile=tile, split_k=1, out_dtype=F32)
        ad, kw = aq[:, :K].view(torch.float8_e4m3fn).float(), dict(row_scale=asc)
    else:
        lin = ops.PackedLinearMX(g["w"], bias=g["bias"])
        aq, asc = ops.quantize_mx_fp8(g["a"])
        run = lambda a8: ops.gemm_mx_fp8(a8, asc, lin, tile=tile, split_k=1, out_dtype=F32)
        ad, kw = ops.mx_dequant(aq, asc, K), {}
    assert aq.dtype == U8 and tuple(aq.shape) == (M, K)
    view, region = place(arena, "gemm_fp8_a", aq)
    out = run(view)
    wd = lin.dequant()
    p, m = kcmp.product_terms(ad, wd)
    trunc = kcmp.f8_mfma_truncation(ad, wd)
    # K products + 2 roundings for the scales, and the MFMA's own named term (tests/test_fp8_gpu.py: dequantised_product)
    ref = kcmp.epilogue_reference((p, m, K + 2, trunc), bias=g["bias"], out_dtype=F32, **kw)["C"]
    check_c(out, ref, what)
    assert_same_bits(out, run(aq), what)
    finish(arena, region, what)


@pytest.mark.parametrize("form", ["rows", "mx"])
def test_gemm_fp8_far_mx_output_copy(dev, arena, form):
    """The MX output copy (mg_epilogue.C8) is dense by contract (ldc8 == ceil(N / 128) * 128), so a far one is a real
    66048 x 65536 output: 4.33 GB of e4m3 codes in the arena, rows from 65536 on past 2^32 bytes; K = 256 keeps it at 2 TFLOP.
    Only the copy is written (no bf16 C), by ops.gemm_fp8 and by ops.gemm_mx_fp8.  Checked rows: 0 .. 63 and 65472 .. 66047 --
    (a) the reference of tests/test_fp8_gpu.py::test_fp8_gemm_writes_the_mx_copy: the copy equals mg_quantize_mx_fp8 of the bf16
    output, codes and block scales, here the output of the same GEMM on those rows alone; (b) is the same comparison; (c) every
    8 bytes of the copy were written (0xFF is no code the quantiser emits for finite values) and nothing outside it."""
    from magma_amd import ops
    Mo, No = far.CASES["gemm_mx_out"].shape
    a = rnd(Mo, K, seed=141).to(dev)
    w = rnd(No, K, scale=0.05, seed=142).to(dev)
    bias = rnd(No, seed=143, dtype=F32).to(dev)
    rows = torch.cat([torch.arange(0, 64), torch.arange(Mo - 576, Mo)]).to(dev)
    if form == "rows":
        lin = ops.PackedLinearFP8(w, bias=bias)
        aq, asc = ops.quantize_rows_fp8(a)
        asc_rows = asc[rows].contiguous()
        gemm8 = ops.gemm_fp8
    else:
        lin = ops.PackedLinearMX(w, bias=bias)
        aq, asc = ops.quantize_mx_fp8(a)
        _, asc_rows = ops.quantize_mx_fp8(a[rows].contiguous())       # block scales are laid out per 64-row group
        gemm8 = ops.gemm_mx_fp8
    q, region = place(arena, "gemm_mx_out")
    sc = torch.full((int(ops.L.load().mg_mx_scale_bytes(Mo, No)),), 0xFF, dtype=U8, device=dev)
    assert q.is_contiguous() and q.stride(0) == No
    assert gemm8(aq, asc, lin, tile=256, mx_out=(q, sc), no_out=True) is None
    ref = gemm8(aq[rows].contiguous(), asc_rows, lin, tile=256)
    rq, rs = ops.quantize_mx_fp8(ref.contiguous())
    assert torch.equal(q[rows], rq[:, :No]), "gemm_fp8, far MX copy: codes"
    got_s, ref_s = ops.mx_scales_rowmajor(sc, Mo, No), ops.mx_scales_rowmajor(rs, rows.numel(), No)
    assert torch.equal(got_s[rows], ref_s), "gemm_fp8, far MX copy: block scales"
    assert not bool((got_s == 0xFF).any()), "gemm_fp8, far MX copy: a block scale was not written"
    words = q.view(torch.int64)
    for r0 in range(0, Mo, 8192):
        assert not bool((words[r0:r0 + 8192] == -1).any()), f"gemm_fp8, far MX copy: rows from {r0} hold unwritten bytes"
    finish(arena, region, "gemm_fp8, far MX copy")


# ---------------------------------------------------------------------------------------------------------------------------
# contiguous KV caches past 4 GiB
# ---------------------------------------------------------------------------------------------------------------------------
KV_ROWS = (0, 127, 128, 129)          # batch row 128 starts at exactly 2^31 elements = 2^32 bytes of either cache
STAGE_SHIFT = far.KV_STAGE_SHIFT      # kv_reorder's staging caches: the same rows, this many positions further on


def test_decode_caches_past_4_gib(dev, arena):
    """K and V [130, 16, 4096, 256] bf16 (4.36 GB each), both in the arena, per-row positions of at most 66: the cache append
    (rotary_split), attn_decode, attn_decode_fused, decode_attn_gemv, attn_prefill_cached (a chunk of 8), kv_broadcast and
    kv_reorder on batch rows 0, 127, 128 and 129 -- (a) rotary_reference for q and the appended key, the decode-attention bound of
    tests/test_kernels_gpu.py and assert_causal_attention for the outputs; (b) the same bits as the same rows in a tight
    four-row cache; (c) nothing outside the two caches written.  The other batch rows hold poison and are not looked at; every
    slot behind a row's context is poison too, so one key too many is NaN.  kv_reorder runs last, its staging caches as views
    into unused positions of the same rows (see there)."""
    from magma_amd import ops
    from oracle.model import rotary_tables
    from test_kernels_gpu import assert_decode_attention
    B, H, Smax = far.KV_B, far.KV_H, far.KV_SMAX
    d, n, ctx_max, T = H * 256, len(KV_ROWS), 80, 8        # ctx_max: one past the last slot any checked row uses
    _, kreg = place(arena, "kv_cache_k")
    _, vreg = place(arena, "kv_cache_v", fresh=False)
    kc, vc = kreg.view(B, H, Smax, 256), vreg.view(B, H, Smax, 256)
    pos_all = [(7 * b) % 65 + 1 for b in range(B)]
    assert max(pos_all) <= 65
    d_pos = torch.tensor(pos_all, dtype=torch.int32, device=dev)
    idx = torch.tensor(KV_ROWS, device=dev)
    near_k = torch.zeros(n, H, Smax, 256, dtype=BF16, device=dev)
    near_v = torch.zeros(n, H, Smax, 256, dtype=BF16, device=dev)
    near_k[:, :, :ctx_max] = rnd(n, H, ctx_max, 256, scale=0.5, seed=121).to(dev)
    near_v[:, :, :ctx_max] = rnd(n, H, ctx_max, 256, seed=122).to(dev)
    for i, b in enumerate(KV_ROWS):
        kc[b, :, :pos_all[b]] = near_k[i, :, :pos_all[b]]
        vc[b, :, :pos_all[b]] = near_v[i, :, :pos_all[b]]
    qkv = rnd(B, 3 * d, scale=0.5, seed=123).to(dev)
    sin_t, cos_t = rotary_tables(64, Smax)
    sin_t, cos_t = sin_t.to(dev).contiguous(), cos_t.to(dev).contiguous()
    qkv_n, pos_n = qkv[idx].contiguous(), d_pos[idx].contiguous()
    # the append
    q = torch.full((B, H, 1, 256), float("nan"), dtype=BF16, device=dev)
    ops.rotary_split(qkv, B, 1, H, 64, sin_t, cos_t, q, kc, vc, d_pos=d_pos, pos_stride=1)
    q_n = torch.full((n, H, 1, 256), float("nan"), dtype=BF16, device=dev)
    ops.rotary_split(qkv_n, n, 1, H, 64, sin_t, cos_t, q_n, near_k, near_v, d_pos=pos_n, pos_stride=1)
    k_far, v_far = kc[idx][:, :, :ctx_max], vc[idx][:, :, :ctx_max]
    assert_same_bits(q[idx], q_n, "rotary_split append, far caches: q")
    ctx_rows = [pos_all[b] + 1 for b in KV_ROWS]
    xd = qkv_n.view(n, 3, H, 1, 256)
    sin_r, cos_r = sin_t[pos_n.long()][:, None, None, :], cos_t[pos_n.long()][:, None, None, :]
    new_k = torch.stack([k_far[i, :, c - 1:c] for i, c in enumerate(ctx_rows)])
    for got, src, name in ((q[idx], xd[:, 0], "q"), (new_k, xd[:, 1], "appended k")):
        kcmp.assert_elementwise(got, *kcmp.rotary_reference(src, sin_r, cos_r, 64), f"rotary_split append, far caches: {name}")
    for i, c in enumerate(ctx_rows):
        assert torch.equal(bits(k_far[i, :, :c]), bits(near_k[i, :, :c])) and torch.equal(bits(v_far[i, :, :c]), bits(near_v[i, :, :c])), \
            f"rotary_split append, far caches: batch row {KV_ROWS[i]}"
        assert bool(torch.isnan(k_far[i, :, c:].float()).all()), f"rotary_split append wrote behind position {c - 1} of row {KV_ROWS[i]}"
    # decode attention over the far caches
    for name, run in (("attn_decode", lambda x, qq, k, v, o, bb, p: ops.attn_decode(qq, k, v, o, bb, H, p, pos_stride=1)),
                      ("attn_decode_fused", lambda x, qq, k, v, o, bb, p: ops.attn_decode_fused(x, k, v, o, bb, H, p, 64, sin_t, cos_t, pos_stride=1))):
        out = torch.full((B, d), float("nan"), dtype=BF16, device=dev)
        run(qkv, q, kc, vc, out, B, d_pos)
        out_n = torch.full((n, d), float("nan"), dtype=BF16, device=dev)
        run(qkv_n, q_n, near_k, near_v, out_n, n, pos_n)
        assert_decode_attention(q_n, near_k, near_v, ctx_rows, f"{name}, far caches", out[idx])
        assert_same_bits(out[idx], out_n, f"{name}, far caches")
    assert torch.equal(bits(kc[idx][:, :, :ctx_max]), bits(k_far)), "the fused append changed the cache"
    # decode_attn_gemv: the fused decode attention beside an independent GEMV (2 x 512 -> 264), same caches
    xg = rnd(2, 512, seed=124).to(dev)
    wg = rnd(264, 512, scale=0.05, seed=125).to(dev)
    ling = ops.PackedLinear(wg, bias=rnd(264, seed=126, dtype=F32).to(dev))
    out3 = torch.full((B, d), float("nan"), dtype=BF16, device=dev)
    y = torch.full((2, 264), float("nan"), dtype=F32, device=dev)
    ops.decode_attn_gemv(qkv, kc, vc, out3, B, H, d_pos, 64, sin_t, cos_t, (xg, ling, y, {"out_dtype": F32}), pos_stride=1)
    out3_n = torch.full((n, d), float("nan"), dtype=BF16, device=dev)
    y_n = torch.full((2, 264), float("nan"), dtype=F32, device=dev)
    ops.decode_attn_gemv(qkv_n, near_k, near_v, out3_n, n, H, pos_n, 64, sin_t, cos_t, (xg, ling, y_n, {"out_dtype": F32}), pos_stride=1)
    assert_decode_attention(q_n, near_k, near_v, ctx_rows, "decode_attn_gemv, far caches", out3[idx])
    assert_same_bits(out3[idx], out3_n, "decode_attn_gemv, far caches")
    kcmp.assert_linear(y, "decode_attn_gemv, far caches: the co-launched GEMV", xg, wg, bias=ling.bias)
    assert_same_bits(y, y_n, "decode_attn_gemv, far caches: the co-launched GEMV")
    assert torch.equal(bits(kc[idx][:, :, :ctx_max]), bits(k_far)), "decode_attn_gemv changed the cache"
    # attn_prefill_cached: a chunk of T = 8 queries per row behind the token just appended; the chunk's keys and values are
    # put into the far caches from the near ones (slots p .. p + T - 1, p = position + 1)
    p2 = d_pos + 1
    p2_n = p2[idx].contiguous()
    for i, b in enumerate(KV_ROWS):
        lo = pos_all[b] + 1
        kc[b, :, lo:lo + T] = near_k[i, :, lo:lo + T]
        vc[b, :, lo:lo + T] = near_v[i, :, lo:lo + T]
    assert max(pos_all) + 1 + T <= ctx_max
    qc = rnd(B, H, T, 256, scale=0.5, seed=127).to(dev)
    qc_n = qc[idx].contiguous()
    outc = torch.full((B * T, d), float("nan"), dtype=BF16, device=dev)
    ops.attn_prefill_cached(qc, kc, vc, outc, B, H, T, p2, pos_stride=1)
    outc_n = torch.full((n * T, d), float("nan"), dtype=BF16, device=dev)
    ops.attn_prefill_cached(qc_n, near_k, near_v, outc_n, n, H, T, p2_n, pos_stride=1)
    outc_sel = outc.view(B, T, d)[idx].reshape(n * T, d)
    kcmp.assert_causal_attention(outc_sel, qc_n, near_k[:, :, :ctx_max], near_v[:, :, :ctx_max], "attn_prefill_cached, far caches", p0=p2_n)
    assert_same_bits(outc_sel, outc_n, "attn_prefill_cached, far caches")
    # kv_broadcast: one position of a source row copied to the other rows of its group of 10; the last group (batch rows 120 ..
    # 129) straddles 2^32 bytes -- once read below and written above it (source 127), once the other way round (source 128).
    # The other groups copy poison onto poison.
    k5, v5 = kreg.view(1, B, H, Smax, 256), vreg.view(1, B, H, Smax, 256)
    for src_row, p in ((127, 3), (128, 5)):
        src = torch.arange(0, B, 10, dtype=torch.int32)
        src[12] = src_row
        want_k, want_v = kc[120:130, :, :ctx_max].clone(), vc[120:130, :, :ctx_max].clone()
        want_k[:, :, p], want_v[:, :, p] = want_k[src_row - 120, :, p].clone(), want_v[src_row - 120, :, p].clone()
        assert not bool(torch.isnan(want_k[:, :, p].float()).any())
        ops.kv_broadcast(k5, v5, 10, src.to(dev), torch.full((B,), p, dtype=torch.int32, device=dev), pos_stride=1)
        assert torch.equal(bits(kc[120:130, :, :ctx_max]), bits(want_k)) and torch.equal(bits(vc[120:130, :, :ctx_max]), bits(want_v)), \
            f"kv_broadcast from batch row {src_row}, far caches"
    # kv_reorder: row b gets positions [0, d_pos[parent[b]]) of row parent[b].  It takes two staging caches of the caches' shape
    # and uses one offset for all four operands; only the first d_pos positions of a row are touched, so the staging caches are
    # views of the arena shifted by 1024 positions: staging position i of a row lies on the unused position 1024 + i of the same
    # row of K / V.  Parents cross batch row 128 both ways: 127 <-> 128 (a swap, both staged), 129 <- 0 and 126 <- 129 (129 is
    # staged too); every other row is its own parent.  A copy, bit for bit: (a) against plain indexing of a snapshot, (b) against
    # the same call on a tight five-row copy with Smax = 128.
    ksv, _ = place(arena, "kv_stage_k", fresh=False)
    vsv, _ = place(arena, "kv_stage_v", fresh=False)
    assert ksv.data_ptr() == kc[0, 0, STAGE_SHIFT].data_ptr() and vsv.data_ptr() == vc[0, 0, STAGE_SHIFT].data_ptr()
    ks5, vs5 = ksv.view(1, B, H, Smax, 256), vsv.view(1, B, H, Smax, 256)
    rows5 = (0, 126, 127, 128, 129)
    moves = {127: 128, 128: 127, 129: 0, 126: 129}                    # destination: parent
    parent = torch.arange(B, dtype=torch.int32)
    for dst_row, src_row in moves.items():
        parent[dst_row] = src_row
    valid = {b: pos_all[b] + 1 + T for b in KV_ROWS}                    # positions of row b that hold data
    cnt = torch.zeros(B, dtype=torch.int32)
    for b, c in valid.items():
        cnt[b] = c
    idx5 = torch.tensor(rows5, device=dev)
    old_k, old_v = kc[idx5][:, :, :ctx_max].clone(), vc[idx5][:, :, :ctx_max].clone()
    want_k, want_v = old_k.clone(), old_v.clone()
    for dst_row, src_row in moves.items():
        i, j, c = rows5.index(dst_row), rows5.index(src_row), valid[src_row]
        want_k[i, :, :c], want_v[i, :, :c] = old_k[j, :, :c], old_v[j, :, :c]
    Sn = 128
    nk, nv, nks, nvs = (torch.full((1, 5, H, Sn, 256), float("nan"), dtype=BF16, device=dev) for _ in range(4))
    nk[0, :, :, :ctx_max], nv[0, :, :, :ctx_max] = old_k, old_v
    parent_n = torch.tensor([rows5.index(int(parent[b])) for b in rows5], dtype=torch.int32, device=dev)
    ops.kv_reorder(nk, nv, nks, nvs, parent_n, cnt[list(rows5)].contiguous().to(dev), pos_stride=1)
    ops.kv_reorder(k5, v5, ks5, vs5, parent.to(dev), cnt.to(dev), pos_stride=1)
    got_k, got_v = kc[idx5][:, :, :ctx_max], vc[idx5][:, :, :ctx_max]
    assert torch.equal(bits(got_k), bits(want_k)) and torch.equal(bits(got_v), bits(want_v)), "kv_reorder, far caches"
    assert torch.equal(bits(got_k), bits(nk[0, :, :, :ctx_max])) and torch.equal(bits(got_v), bits(nv[0, :, :, :ctx_max])), \
        "kv_reorder, far caches: the near copy gives other bits"
    for b in (127, 128, 129):                                           # the staged rows: their own positions, nothing behind
        i, c = rows5.index(b), valid[b]
        st_k, st_v = kc[b, :, STAGE_SHIFT:STAGE_SHIFT + ctx_max], vc[b, :, STAGE_SHIFT:STAGE_SHIFT + ctx_max]
        assert torch.equal(bits(st_k[:, :c]), bits(old_k[i, :, :c])) and torch.equal(bits(st_v[:, :c]), bits(old_v[i, :, :c])), \
            f"kv_reorder, far caches: staging of batch row {b}"
        assert bool(torch.isnan(st_k[:, c:].float()).all()) and bool(torch.isnan(st_v[:, c:].float()).all())
    # (c): the staged rows' staging positions wiped, every position from ctx_max on, in every row of both caches (the staging of
    # every other row with them), and the rest of the arena, is still poison
    torch.cuda.synchronize()
    far.wipe(kc[:, :, :ctx_max], vc[:, :, :ctx_max])
    far.wipe(kc[127:130, :, STAGE_SHIFT:STAGE_SHIFT + ctx_max], vc[127:130, :, STAGE_SHIFT:STAGE_SHIFT + ctx_max])
    far.assert_arena_poison(arena, "decode over far caches")


# ---------------------------------------------------------------------------------------------------------------------------
# refusals of the attention launchers
# ---------------------------------------------------------------------------------------------------------------------------
def test_row_attention_refuses_rows_past_its_32_bit_offsets(dev, arena):
    """attn_fwd_rows / attn_bwd_rows keep 32-bit byte offsets inside one (batch, head): S * ld_row * 2 >= 2^31 is refused."""
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    far.poison(arena)
    S, ld = 64, 2 ** 24
    assert S * ld * 2 == 2 ** 31
    qkv, _ = far.far_view(arena, BF16, (S, 768), (ld, 1))
    p = qkv.data_ptr()
    x = ops.AttnRows(p, p + 512, p + 1024, ld, S * ld, 256, 1, 1, S, keep=(arena,))
    out = torch.zeros(S, 256, dtype=BF16, device=dev)
    lse = torch.zeros(1, 1, S, dtype=F32, device=dev)
    with pytest.raises(MagmaHipError, match="S \\* ld_row exceeds the 32-bit byte offsets"):
        ops.attn_fwd_rows(x, out, lse)
    dO = torch.zeros(1, 1, S, 256, dtype=BF16, device=dev)
    with pytest.raises(MagmaHipError, match="S \\* ld_row exceeds the 32-bit byte offsets"):
        ops.attn_bwd_rows(x, dO, out, lse)
    torch.cuda.synchronize()
    assert not bool(out.any()), "a refused launch wrote its output"
    far.assert_arena_poison(arena, "refused row attention")


def test_cached_prefill_refuses_a_cache_past_its_32_bit_offsets(dev, arena):
    """attn_prefill_cached / attn_prefill_tree: Smax * 256 * 2 >= 2^31 (Smax = 2^22) is refused."""
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    far.poison(arena)
    Smax, T = 2 ** 22, 8
    kc, lay = far.far_view(arena, BF16, (1, 1, Smax, 256), (Smax * 256, Smax * 256, 256, 1))
    vc, _ = far.far_view(arena, BF16, (1, 1, Smax, 256), (Smax * 256, Smax * 256, 256, 1), skew=lay.span)
    q = torch.zeros(1, 1, T, 256, dtype=BF16, device=dev)
    out = torch.zeros(T, 256, dtype=BF16, device=dev)
    d_pos = torch.full((1,), 4, dtype=torch.int32, device=dev)
    with pytest.raises(MagmaHipError, match="Smax exceeds the 32-bit byte offsets"):
        ops.attn_prefill_cached(q, kc, vc, out, 1, 1, T, d_pos)
    sub = torch.full((1, T), T, dtype=torch.int32, device=dev)
    with pytest.raises(MagmaHipError, match="Smax exceeds the 32-bit byte offsets"):
        ops.attn_prefill_tree(q, kc, vc, out, 1, 1, T, d_pos, sub, p_min=4)
    torch.cuda.synchronize()
    assert not bool(out.any()), "a refused launch wrote its output"
    far.assert_arena_poison(arena, "refused cached prefill")
