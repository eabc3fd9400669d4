"""The 3x3 convolutions of the CLIP ResNet trunk, pass by pass and per element: forward, input gradient (dgrad), weight gradient
(wgrad), and the layout kernels between them.

Three pieces of hand-written code serve only these convolutions: the implicit-im2col A loader of gemm128_kernel (MG_A_CONV3X3,
csrc/gemm.hip), im2col_t_kernel (csrc/backward.hip), and the chain train_engine.py::_unit_bwd builds from them.  The whole-model
gradient tests see them through rel-L2 norms of weight gradients that sum over B*H*W pixels: one wrong halo column moves such a
norm by about 1 / W.  Here every output element is compared, in two input families (tests/kernel_compare.py: conv_case):

  "integers"   operands in [-4, 4], scales in {0.5, 1, 2}, gates in {-1, 0, 1}: every partial sum is exact in fp32 in any order
               (assert_exact_in_fp32 checks the premise per case), so the output must EQUAL the fp64 reference cast once --
               a flipped tap, a halo leak, a dropped or doubled K chunk, a wrong split start fail outright;
  "gaussian"   the suite's usual operands against the per-element bounds of epilogue_reference.

tests/test_kernel_compare_cpu.py runs both comparisons against honest stand-ins and against the seeded faults, at these shapes.

Which case reaches which mechanism (cpt = channels / 8 = 16-byte chunks per tap; a K-tile holds 8 chunks; M-tiles of 128 rows):
  a split start inside a tap        2x9x15,72->40 forward, split_k 0 / 2 (chunk 48 of cpt 9) and 5 (chunks 24, 48; 72 is a tap
                                    boundary); its dgrad (40 channels, cpt 5) at split_k 2 (chunk 24) and 5 (chunks 16, 32);
                                    1x12x12,192->136 dgrad (136 channels, cpt 17) at every split count; 2x12x12,768->768 at 16 splits
  a tap boundary inside a K-tile    every shape but 1x12x12,192->136 forward and 768->768 (cpt 24 and 96 are multiples of 8)
  a batch boundary inside an M-tile 3x5x7 (rows 35, 70), 2x9x15 (row 135 in the second tile), 2x12x12 (row 144 in the second tile),
                                    2x1x5 and 2x5x1 (row 5)
  a 1-pixel image                   1x1x1; one pixel high 2x1x5; one pixel wide 2x5x1
  M % 8 != 0 in wgrad               M = 1, 10, 10, 105, 270: the GEMM contracts over round_up(M, 8) columns of both operands
  Cin > 64 in im2col_t              72 (a second channel block of 8), 192 (three full blocks), 768
  the four dgrad epilogue forms     DGRAD_FORMS, at every shape and split count

Split counts follow gemm_dispatch (kernel_compare.gemm128_splits restates its rule, FWD_SPLITS / DGRAD_SPLITS spell the result
out) and are OBSERVED: the split-K workspace is filled with NaN before a call, and slab s was written iff its first element no
longer is one."""
import pytest
import torch
import torch.nn.functional as F

import kernel_compare as kcmp

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
SENT = 7.0
SHAPES = kcmp.CONV_SHAPES
IDS = [kcmp.conv_shape_id(s) for s in SHAPES]
FORCED = {(2, 9, 15, 72, 40), (1, 12, 12, 192, 136)}          # the shapes that also run split_k = 5

# split_k -> slabs of the forward call (M = B H W, N = Cout, K = 9 Cin).  split_k 0 on fewer than 8 K-tiles does not split (the
# automatic rule wants 4 K-tiles per split): those cases run the unsplit kernel a second time, through the branch of the
# dispatch that was handed a workspace -- said here, not hidden -- and split_k 2 is forced on every shape so that each of them
# also runs split.
FWD_SPLITS = {
    (1, 1, 1, 8, 8): {1: 1, 0: 1, 2: 2},                      # 2 K-tiles
    (2, 1, 5, 24, 16): {1: 1, 0: 1, 2: 2},                    # 4 K-tiles
    (2, 5, 1, 24, 16): {1: 1, 0: 1, 2: 2},
    (3, 5, 7, 40, 24): {1: 1, 0: 1, 2: 2},                    # 6 K-tiles: 3 + 3, the second split starts at chunk 24 of cpt 5
    (2, 9, 15, 72, 40): {1: 1, 0: 2, 2: 2, 5: 4},             # 11 K-tiles: 6 + 5; a 5-way request gives 3 + 3 + 3 + 2
    (1, 12, 12, 192, 136): {1: 1, 0: 6, 2: 2, 5: 5},          # 27 K-tiles, 4 output tiles
    (2, 12, 12, 768, 768): {1: 1, 0: 16, 2: 2},               # 108 K-tiles, 18 output tiles: 15 x 7 + 3
}
# the dgrad call of the same convolution: the loader walks the Cout channels of the upstream gradient (N = Cin, K = 9 Cout)
DGRAD_SPLITS = {
    (1, 1, 1, 8, 8): {1: 1, 0: 1, 2: 2},
    (2, 1, 5, 24, 16): {1: 1, 0: 1, 2: 2},                    # 16 channels: 3 K-tiles, 2 + 1
    (2, 5, 1, 24, 16): {1: 1, 0: 1, 2: 2},
    (3, 5, 7, 40, 24): {1: 1, 0: 1, 2: 2},                    # 24 channels: 4 K-tiles
    (2, 9, 15, 72, 40): {1: 1, 0: 1, 2: 2, 5: 3},             # 40 channels: 6 K-tiles; a 5-way request gives 2 + 2 + 2
    (1, 12, 12, 192, 136): {1: 1, 0: 5, 2: 2, 5: 5},          # 136 channels: K = 1224, 20 K-tiles with a partial last one
    (2, 12, 12, 768, 768): {1: 1, 0: 16, 2: 2},
}

_cases = {}


def case(dev, family, shape):
    """Operands and fp64 product terms of one (family, shape), made once and left unchanged."""
    key = (family, tuple(shape))
    if key not in _cases:
        _cases[key] = kcmp.conv_case(family, shape, device=dev)
    return _cases[key]


def terms(c, name, make):
    if name not in c:
        c[name] = make()
    return c[name]


def padded_out(M, N, dtype, dev):
    """[M, N] view inside a [M + 2, round_up(N, 8) + 8] buffer of SENT."""
    buf = torch.full((M + 2, (N + 7) // 8 * 8 + 8), SENT, dtype=dtype, device=dev)
    return buf, buf[:M, :N]


def assert_untouched(buf, M, N, what):
    assert bool((buf[M:] == SENT).all()) and bool((buf[:M, N:] == SENT).all()), f"{what}: wrote outside [0, M) x [0, N)"


def run_observing_splits(ops, dev, M, N, call):
    """call() with the split-K workspace prefilled with NaN -> (result, number of slabs that were written)."""
    ws = ops.splitk_workspace(dev)
    ldws = (N + 127) // 128 * 128
    assert 17 * M * ldws <= ws.numel()
    ws[: 17 * M * ldws].fill_(float("nan"))
    out = call()
    first = ws[: 17 * M * ldws: M * ldws]
    written = ~torch.isnan(first)
    n = int(written.sum())
    assert bool(written[:n].all()), "the written slabs are not the first ones"
    return out, max(n, 1)


def exact_top(mag, *more):
    """Magnitude sum of a whole epilogue for the exactness premise: the product at scale <= 2, and the terms added to it."""
    top = 2.0 * mag
    for t in more:
        top = top + kcmp.f64(t).abs()
    return top


def split_list(shape):
    return (1, 0, 2, 5) if tuple(shape) in FORCED else (1, 0, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", kcmp.CONV_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_conv3x3_forward(dev, shape, family):
    """ops.gemm(x_nhwc, PackedLinear, conv=(H, W, Cin)) as image_encoders.py::_conv calls it: bare, and with the bottleneck's
    whole epilogue (folded-BN scale and bias, ReLU, one residual, ReLU after); both weight layouts; unsplit, automatic and
    forced split-K."""
    from magma_amd import ops
    B, H, W, Cin, Cout = shape
    c = case(dev, family, shape)
    M = c["M"]
    prod = terms(c, "fwd", lambda: kcmp.conv2d_terms(c["x"], c["w"]))
    lin = ops.PackedLinear(kcmp.conv_weight_rows(c["w"]), bias=c["bias"], tiled=True, rowmajor=True)
    refs = {"bare": kcmp.epilogue_reference(prod)["C"],
            "full": kcmp.epilogue_reference(prod, scale=c["scale"], bias=c["bias"], act="relu", residuals=(c["res_out"],), act_after="relu")["C"]}
    tops = {"bare": prod[1], "full": exact_top(prod[1], c["bias"], c["res_out"])}
    kws = {"bare": dict(use_bias=False),
           "full": dict(scale=c["scale"], act=ops.MG_ACT_RELU, residuals=(c["res_out"],), act_after=ops.MG_ACT_RELU)}
    for layout in ("rm", "ft"):
        for sk in split_list(shape):
            assert kcmp.gemm128_splits(M, Cout, 9 * Cin, sk) == FWD_SPLITS[tuple(shape)][sk]
            for ep in ("bare", "full"):
                what = f"conv3x3 forward {kcmp.conv_shape_id(shape)} {family} {layout} split_k={sk} {ep}"
                buf, view = padded_out(M, Cout, BF16, dev)
                _, slabs = run_observing_splits(ops, dev, M, Cout, lambda: ops.gemm(c["x_rows"], lin, out=view, conv=(H, W, Cin), layout=layout,
                                                                                    split_k=sk, **kws[ep]))
                assert slabs == FWD_SPLITS[tuple(shape)][sk], f"{what}: {slabs} split-K slabs were written"
                kcmp.assert_conv_output(family, view, refs[ep], what, mag=tops[ep])
                assert_untouched(buf, M, Cout, what)


# ---------------------------------------------------------------------------------------------------------------------------
# dgrad
# ---------------------------------------------------------------------------------------------------------------------------
# (name, gate?, aux_after, residual?): the 2 x 2 of gate position and residual, and the two calls without a gate that
# _encoder_backward also issues (the shortcut / conv3 of a strided block; conv1 of the first block)
DGRAD_FORMS = [("gate", True, False, False), ("gate + residual", True, False, True), ("gate after", True, True, False),
               ("residual, gate after", True, True, True), ("plain", False, False, False), ("residual", False, False, True)]


@pytest.mark.parametrize("family", kcmp.CONV_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_conv3x3_dgrad(dev, shape, family):
    """_unit_bwd's input gradient: conv_weight_relayout(w, 1, scale), then the conv GEMM over the upstream gradient with the ReLU
    gate and the identity-path residual in its epilogue.  The loader walks the Cout channels here (8, 16, 24, 40, 136, 768).
    Reference: the fp64 input gradient of conv2d(x, w * scale[co], padding = 1) with w * scale as the re-layout wrote it, gated and
    summed in the order of the epilogue contract."""
    from magma_amd import ops
    B, H, W, Cin, Cout = shape
    c = case(dev, family, shape)
    M = c["M"]
    dg = ops.conv_weight_relayout(c["w"], 1, c["scale"])
    assert torch.equal(dg[:, : 9 * Cout], kcmp.conv_dgrad_weight_rows(c["w"], c["scale"])) and bool((dg[:, 9 * Cout:] == 0).all())
    prod = terms(c, "dgrad", lambda: kcmp.conv2d_dgrad_terms(c["g"], wd=dg))
    if family == "integers":       # w * scale is exact in bf16 there: the terms from w and scale are the same numbers
        ref_w = kcmp.conv2d_dgrad_terms(c["g"], c["w"], c["scale"])
        assert torch.equal(prod[0], ref_w[0])
    wop = ops.RawWeight(dg, K=9 * Cout)
    for name, gated, after, with_res in DGRAD_FORMS:
        res = (c["res_in"],) if with_res else ()
        ref = kcmp.epilogue_reference(prod, aux=c["gate_in"] if gated else None, aux_mode="relu_gate" if gated else "none", aux_after=after,
                                      residuals=res)["C"]
        kw = dict(aux=c["gate_in"], aux_mode=ops.MG_AUX_RELU_GATE, aux_after=after) if gated else {}
        for sk in split_list(shape):
            assert kcmp.gemm128_splits(M, Cin, 9 * Cout, sk) == DGRAD_SPLITS[tuple(shape)][sk]
            what = f"conv3x3 dgrad {kcmp.conv_shape_id(shape)} {family} split_k={sk} {name}"
            buf, view = padded_out(M, Cin, BF16, dev)
            _, slabs = run_observing_splits(ops, dev, M, Cin, lambda: ops.gemm(c["g_rows"], wop, out=view, conv=(H, W, Cout), layout="rm",
                                                                               use_bias=False, residuals=res, split_k=sk, **kw))
            assert slabs == DGRAD_SPLITS[tuple(shape)][sk], f"{what}: {slabs} split-K slabs were written"
            kcmp.assert_conv_output(family, view, ref, what, mag=exact_top(prod[1], *res))
            assert_untouched(buf, M, Cin, what)
            if gated and after:      # a closed gate after the residual sum: exactly zero
                assert bool((view[c["gate_in"].float() <= 0] == 0).all()), what


# ---------------------------------------------------------------------------------------------------------------------------
# wgrad
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", kcmp.CONV_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_conv3x3_wgrad(dev, shape, family):
    """_unit_bwd's weight gradient: g^T from transpose and from transpose_bn_param_grad, x^T from im2col_t, then the accumulating fp32
    GEMM with row_scale onto a non-zero gradient buffer (_acc_wgrad's in-place branch) and the temporary + scale_rows_acc
    branch.  Reference: base + scale[co] * dW, dW the fp64 weight gradient of the convolution."""
    from magma_amd import ops
    B, H, W, Cin, Cout = shape
    c = case(dev, family, shape)
    M = c["M"]
    Mp = (M + 7) // 8 * 8
    g_rows, scale, base = c["g_rows"], c["scale"], c["base"]
    gT_ref = torch.zeros(Cout, Mp, dtype=BF16, device=dev)
    gT_ref[:, :M] = g_rows.t()
    gT = ops.transpose(g_rows)
    assert torch.equal(gT, gT_ref)
    gen = torch.Generator().manual_seed(M + Cout)
    y, sub = (torch.randint(-4, 5, (M, Cout), generator=gen).to(BF16).to(dev) for _ in range(2))
    gamma, beta = torch.full((Cout,), 2.0, device=dev), torch.ones(Cout, device=dev)
    dgamma, dbeta = torch.zeros(Cout, device=dev), torch.zeros(Cout, device=dev)
    gT2 = ops.transpose_bn_param_grad(g_rows, y, sub, gamma, beta, dgamma, dbeta)
    assert torch.equal(gT2, gT_ref)
    g64 = g_rows.double()
    db_ref, db_mag = g64.sum(0), g64.abs().sum(0)
    kcmp.assert_elementwise(dbeta, db_ref, kcmp.rounded(db_ref, kcmp.gamma(M + 8) * db_mag, F32), f"transpose_bn_param_grad dbeta {M}x{Cout}")
    xT = ops.im2col_t(c["x_rows"], B, H, W, Cin)
    assert torch.equal(xT, kcmp.im2col_t_reference(c["x"]))
    prod = terms(c, "wgrad", lambda: kcmp.conv2d_wgrad_terms(g_rows, c["x"]))
    ref = kcmp.epilogue_reference(prod, row_scale=scale, base=base, out_dtype=F32)["C"]
    top = exact_top(prod[1], base)
    tag = f"conv3x3 wgrad {kcmp.conv_shape_id(shape)} {family}"
    for name, g_t in (("transpose", gT), ("transpose_bn_param_grad", gT2)):
        grad = base.clone()
        ops.gemm(g_t, ops.RawWeight(xT), out=grad, layout="rm", use_bias=False, accumulate=True, row_scale=scale)
        kcmp.assert_conv_output(family, grad, ref, f"{tag} in place, g^T from {name}", mag=top)
    tmp = ops.gemm(gT, ops.RawWeight(xT), out_dtype=F32, layout="rm", use_bias=False)
    grad = base.clone()
    ops.scale_rows_acc(grad, tmp[:, : 9 * Cin], scale)
    kcmp.assert_conv_output(family, grad, ref, f"{tag} temporary + scale_rows_acc", mag=top)


# ---------------------------------------------------------------------------------------------------------------------------
# the layout kernels on their own: what they write, and what they leave alone
# ---------------------------------------------------------------------------------------------------------------------------
def nan_filled(rows, ld, dev):
    return torch.full((rows, ld), float("nan"), dtype=BF16, device=dev)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_im2col_t_writes_its_contract_and_nothing_else(dev, shape):
    """mg_im2col_t_bf16 into a NaN-filled buffer with ldo > round_up(M, 8): columns < M hold the transposed patches (== F.unfold),
    [M, round_up(M, 8)) hold zeros -- the wgrad GEMM contracts over them -- and everything beyond still holds the fill."""
    from magma_amd import ops
    B, H, W, Cin, Cout = shape
    c = case(dev, "gaussian", shape)
    M = c["M"]
    Mp = (M + 7) // 8 * 8
    out = nan_filled(9 * Cin, Mp + 16, dev)
    ops.check(ops.L.load().mg_im2col_t_bf16(c["x_rows"].data_ptr(), out.data_ptr(), out.stride(0), B, H, W, Cin, ops._stream()), "mg_im2col_t_bf16")
    ref = kcmp.im2col_t_reference(c["x"])
    unf = F.unfold(c["x"].float(), 3, padding=1).permute(1, 0, 2).reshape(9 * Cin, M)
    assert torch.equal(ref[:, :M].float(), unf) and bool((ref[:, M:] == 0).all())
    assert torch.equal(out[:, :Mp], ref), "patches or zero tail"
    assert bool(torch.isnan(out[:, Mp:]).all()), "wrote past round_up(M, 8)"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_transpose_writes_its_contract_and_nothing_else(dev, shape):
    """mg_transpose_bf16 of the upstream gradient [R = B H W, C = Cout] into a NaN-filled buffer, R % 8 != 0 included: columns < R
    hold the transpose, [R, round_up(R, 8)) zeros, the rest the fill; mg_transpose_bn_param_grad_bf16 writes the same bits."""
    from magma_amd import ops
    c = case(dev, "gaussian", shape)
    g = c["g_rows"]
    R, Cc = g.shape
    Rp = (R + 7) // 8 * 8
    for fused in (False, True):
        out = nan_filled(Cc, Rp + 16, dev)
        if fused:
            gamma, beta = torch.ones(Cc, device=dev), torch.zeros(Cc, device=dev)
            dgamma, dbeta = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
            ops.check(ops.L.load().mg_transpose_bn_param_grad_bf16(g.data_ptr(), g.stride(0), out.data_ptr(), out.stride(0), R, Cc, g.data_ptr(), None,
                                                                   gamma.data_ptr(), beta.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                                                   ops._stream()), "mg_transpose_bn_param_grad_bf16")
        else:
            ops.check(ops.L.load().mg_transpose_bf16(g.data_ptr(), g.stride(0), 0, out.data_ptr(), out.stride(0), 0, R, Cc, 1, ops._stream()),
                      "mg_transpose_bf16")
        assert torch.equal(out[:, :R], g.t()), fused
        assert bool((out[:, R:Rp] == 0).all()), f"tail columns [R, round_up(R, 8)) not zero (fused={fused})"
        assert bool(torch.isnan(out[:, Rp:]).all()), f"wrote past round_up(R, 8) (fused={fused})"


# ---------------------------------------------------------------------------------------------------------------------------
# the trunk's element-wise kernels, at one pixel quad, a ragged shape and the trunk's own
# ---------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 2, 2, 8), (3, 6, 10, 264), (2, 14, 14, 3072)]


def pool_operand(family, shape, seed, dev, gate=False):
    gen = torch.Generator().manual_seed(seed)
    if family == "integers":
        t = torch.randint(-1, 2, shape, generator=gen) if gate else torch.randint(-4, 5, shape, generator=gen)
        return t.to(BF16).to(dev)
    t = torch.randn(*shape, generator=gen)
    if gate:
        t.view(-1)[0], t.view(-1)[-1] = 0.0, -0.0
    return t.to(BF16).to(dev)


def assert_map(family, got, ref, mag, n_ops, what):
    if family == "integers":
        kcmp.assert_bit_exact(got, ref, what)
    else:
        kcmp.assert_elementwise(got, ref, kcmp.map_bound(ref, mag, n_ops, got.dtype), what)


@pytest.mark.parametrize("family", kcmp.CONV_FAMILIES)
@pytest.mark.parametrize("B,H,W,C", POOL_SHAPES)
def test_avgpool2_forward_and_backward(dev, B, H, W, C, family):
    """avgpool2: 0.25 * (sum of the 2 x 2 quad), NHWC; avgpool2_bwd: every input pixel gets dy / 4, zero where the gate is closed.
    In the integers family quarters of sums below 16 are bf16 values: equality."""
    from magma_amd import ops
    x = pool_operand(family, (B, H, W, C), 301, dev)
    x64 = x.double().permute(0, 3, 1, 2)
    ref = F.avg_pool2d(x64, 2).permute(0, 2, 3, 1)
    mag = F.avg_pool2d(x64.abs(), 2).permute(0, 2, 3, 1)
    assert_map(family, ops.avgpool2(x), ref, mag, 4, f"avgpool2 {B}x{H}x{W}x{C} {family}")
    dy = pool_operand(family, (B, H // 2, W // 2, C), 302, dev)
    gate = pool_operand(family, (B, H, W, C), 303, dev, gate=True)
    dx_ref = (dy.double() / 4).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert_map(family, ops.avgpool2_bwd(dy, B, H, W, C), dx_ref, dx_ref.abs(), 1, f"avgpool2_bwd {B}x{H}x{W}x{C} {family}")
    gated = dx_ref * (gate.double() > 0)
    got = ops.avgpool2_bwd(dy, B, H, W, C, gate=gate)
    assert_map(family, got, gated, gated.abs(), 1, f"avgpool2_bwd gated {B}x{H}x{W}x{C} {family}")
    assert bool((got[gate.float() <= 0] == 0).all())


@pytest.mark.parametrize("family", kcmp.CONV_FAMILIES)
@pytest.mark.parametrize("B,H,W,C", POOL_SHAPES)
def test_add_gate_operand_combinations(dev, B, H, W, C, family):
    """add_gate: out = (a [+ b]) [* (gate > 0)] over flat tensors of the pool shapes' element counts, all four combinations."""
    from magma_amd import ops
    n = B * H * W * C
    a, b = pool_operand(family, (n,), 311, dev), pool_operand(family, (n,), 312, dev)
    gate = pool_operand(family, (n,), 313, dev, gate=True)
    for with_b in (False, True):
        for with_gate in (False, True):
            ref = a.double() + (b.double() if with_b else 0.0)
            mag = a.double().abs() + (b.double().abs() if with_b else 0.0)
            if with_gate:
                open_ = (gate.double() > 0).double()
                ref, mag = ref * open_, mag * open_
            got = ops.add_gate(a, b if with_b else None, gate if with_gate else None)
            assert_map(family, got, ref, mag, 1, f"add_gate n={n} b={with_b} gate={with_gate} {family}")


@pytest.mark.parametrize("family", kcmp.CONV_FAMILIES)
@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (3, 6, 10)])
def test_stem_im2col(dev, B, H, W, family):
    """stem_im2col: the 3x3 / stride 2 / padding 1 patches of an NCHW image, [B (H/2) (W/2), 32] with column c * 9 + ky * 3 + kx and
    the columns 27..31 zero -- a copy: equal to F.unfold in both families."""
    from magma_amd import ops
    img = pool_operand(family, (B, 3, H, W), 321, dev)
    cols = ops.stem_im2col(img)
    ref = F.unfold(img.float(), 3, padding=1, stride=2).permute(0, 2, 1).reshape(-1, 27)
    assert cols.shape == (B * (H // 2) * (W // 2), 32)
    assert torch.equal(cols[:, :27].float(), ref) and bool((cols[:, 27:] == 0).all())


def test_refusals(dev):
    """Shapes the kernels cannot run are refused by the entry points, not launched."""
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    z = lambda *s: torch.zeros(*s, dtype=BF16, device=dev)
    lib = ops.L.load()
    with pytest.raises(MagmaHipError):                          # odd H
        ops.avgpool2(z(1, 3, 2, 8))
    with pytest.raises(MagmaHipError):                          # odd W
        ops.avgpool2(z(1, 2, 3, 8))
    with pytest.raises(MagmaHipError):                          # C % 8 != 0
        ops.avgpool2(z(1, 2, 2, 12))
    with pytest.raises(MagmaHipError):                          # odd H of the input size
        ops.avgpool2_bwd(z(1, 1, 1, 8), 1, 3, 2, 8)
    with pytest.raises(MagmaHipError):                          # C % 8 != 0
        ops.avgpool2_bwd(z(1, 1, 1, 12), 1, 2, 2, 12)
    with pytest.raises(MagmaHipError):                          # element count not a multiple of 8
        ops.add_gate(z(12))
    with pytest.raises(MagmaHipError):                          # odd H
        ops.stem_im2col(z(1, 3, 3, 2))
    with pytest.raises(MagmaHipError):                          # Cin % 8 != 0
        ops.im2col_t(z(16, 12), 1, 4, 4, 12)
    out = z(72, 16)
    with pytest.raises(MagmaHipError):                          # ldo < round_up(M, 8): M = 20 needs 24
        ops.check(lib.mg_im2col_t_bf16(z(20, 8).data_ptr(), out.data_ptr(), 16, 1, 4, 5, 8, ops._stream()), "mg_im2col_t_bf16")
    with pytest.raises(MagmaHipError):                          # ldo not a multiple of 8
        ops.check(lib.mg_im2col_t_bf16(z(20, 8).data_ptr(), z(72, 28).data_ptr(), 28, 1, 4, 5, 8, ops._stream()), "mg_im2col_t_bf16")
    with pytest.raises(MagmaHipError):                          # C % 8 != 0
        ops.transpose(z(16, 12))
    with pytest.raises(MagmaHipError):                          # ld_out < round_up(R, 8): R = 20 needs 24
        ops.transpose(z(20, 8), out=z(8, 16))
