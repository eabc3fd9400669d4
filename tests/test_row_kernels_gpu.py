"""The one-workgroup-per-row kernels at their edges: LayerNorm forward (one-row and four-rows-per-workgroup forms) and backward,
the cross-entropy head (row losses, mean and count, d logits), greedy argmax, the embedding gather and build_labels.

Every floating-point result is compared per element with an fp64 reference of the same operation against a bound derived from
the kernel's arithmetic (tests/kernel_compare.py; the bounds themselves are checked on the CPU, on the same value families, in
tests/test_kernel_compare_cpu.py); integer results and plain copies bit for bit.  The shapes are the ones at which the kernels
change what they do: one lane of data, 255 / 256 / 257 vectors of a 256-thread loop, the register limits, one row more than a
workgroup's share, the vocabulary of the real head inside its padded buffer.

Operands are views of wider / longer parents filled with a trap value, the way the engines hand them over (``buf[:, :V]`` of a
[R, Vp] buffer, ``take(...)`` views): a kernel that reads a pad column gets NaN / 1e30 / +inf into its result, and after every
call the parent must be bit-identical outside the operand.  Outputs the caller allocates are pre-filled with NaN (integers:
a sentinel), so an element that is not written fails."""
import math

import pytest
import torch

import kernel_compare as kcmp

pytestmark = pytest.mark.gpu

BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64
NAN = float("nan")
EPS = 1e-5


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bits(t):
    """The tensor as integers of its element size: NaN == NaN, -0.0 != 0.0."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def framed(data, ld, trap, dev, pre=3, post=2):
    """data [rows, d] (CPU) inside a parent [pre + rows + post, ld] filled with ``trap`` -> (parent, view, snapshot of the parent)."""
    rows, d = data.shape
    assert ld >= d
    parent = torch.full((pre + rows + post, ld), trap, dtype=data.dtype, device=dev)
    view = parent[pre:pre + rows, :d]
    view.copy_(data)
    return parent, view, parent.clone()


def framed_out(rows, d, ld, dtype, dev, fill=NAN, pre=3, post=2):
    parent = torch.full((pre + rows + post, ld), fill, dtype=dtype, device=dev)
    return parent, parent[pre:pre + rows, :d]


def assert_frame_untouched(parent, view, fill, what):
    """Everything of ``parent`` outside ``view`` still holds ``fill``, bit for bit."""
    rows, d = view.shape
    pre = (view.data_ptr() - parent.data_ptr()) // (parent.element_size() * parent.stride(0))
    outside = torch.ones(parent.shape, dtype=torch.bool, device=parent.device)
    outside[pre:pre + rows, :d] = False
    want = torch.full((1,), fill, dtype=parent.dtype, device=parent.device)
    bad = (bits(parent) != bits(want)) & outside
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the operand were written, first at {bad.nonzero()[0].tolist()}"


def assert_unchanged(parent, snapshot, what):
    assert torch.equal(bits(parent), bits(snapshot)), f"{what}: an input (or the memory around it) was written"


def framed_vec(v, trap, dev, pre=8, post=8):
    """A 1-D operand inside a longer parent (pre elements of ``trap`` before it, post after; pre * itemsize is a multiple of 16)."""
    parent = torch.full((pre + v.numel() + post,), trap, dtype=v.dtype, device=dev)
    parent[pre:pre + v.numel()] = v
    return parent, parent[pre:pre + v.numel()], parent.clone()


def poison_allocator(shape, dtype, dev, n=3):
    """Best effort for outputs an op allocates itself: blocks of that size that were just freed hold NaN."""
    ts = [torch.full(shape, NAN, dtype=dtype, device=dev) for _ in range(n)]
    del ts


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm forward
# ---------------------------------------------------------------------------------------------------------------------------
def ln_params(d, dev, seed):
    g = rnd(d, seed=seed) * 0.1 + 1
    b = rnd(d, seed=seed + 1) * 0.1 + 0.25
    gp, g, gs = framed_vec(g, NAN, dev)
    bp, b, bs = framed_vec(b, NAN, dev)
    return g, b, ((gp, gs), (bp, bs))


def run_layernorm(x_cpu, dev, what, seed=50):
    """ops.layernorm on x inside a NaN-filled parent (ld = d + 24) into a strided, NaN-filled ``out=`` (ld = d + 24), per element
    against the fp64 reference -> (out view, x view, g, b)."""
    from magma_amd import ops
    rows, d = x_cpu.shape
    xp, x, xs = framed(x_cpu, d + 24, NAN, dev)
    g, b, vecs = ln_params(d, dev, seed)
    op, out = framed_out(rows, d, d + 24, BF16, dev)
    ret = ops.layernorm(x, g, b, EPS, out=out)
    assert ret is out
    T = kcmp.layernorm_terms(x, g, b, EPS)
    kcmp.assert_elementwise(out, T["ref"], kcmp.layernorm_bound(T, d), f"layernorm {what} {rows}x{d}")
    assert_frame_untouched(op, out, NAN, f"layernorm {what} out")
    assert_unchanged(xp, xs, f"layernorm {what} x")
    for p, s in vecs:
        assert_unchanged(p, s, f"layernorm {what} gamma / beta")
    return out, x, g, b


ONE_ROW_SHAPES = [(1, 8), (3, 16), (5, 2040), (5, 2048), (5, 2056), (2, 16376), (2, 16384)]
# >= 8192 rows and d <= 4096: four rows per workgroup; (8192, 4104) is wider than that form takes and runs one row per workgroup
MULTI_ROW_SHAPES = [(8193, 8), (8192, 2048), (8195, 2056), (8193, 4096), (8192, 4104)]


@pytest.mark.parametrize("rows,d", ONE_ROW_SHAPES)
def test_layernorm_shape_ladder(dev, rows, d):
    """One lane of data, 255 / 256 / 257 vectors (one and two per thread), the last width below and the width at LN_MAXV."""
    from magma_amd import ops
    x = (rnd(rows, d, seed=41) * 2 + 0.3).to(BF16)
    out, xv, g, b = run_layernorm(x, dev, "ladder")
    assert torch.equal(bits(ops.layernorm(xv, g, b, EPS)), bits(out)), "the op's own contiguous output differs from the strided one"


def test_layernorm_refuses_what_it_cannot_hold(dev):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    for d in (16392, 12):
        with pytest.raises(MagmaHipError):
            ops.layernorm(torch.zeros(2, d, dtype=BF16, device=dev), torch.ones(d, device=dev), torch.zeros(d, device=dev))


@pytest.mark.parametrize("rows,d", MULTI_ROW_SHAPES)
def test_layernorm_rows_per_workgroup_edges(dev, rows, d):
    """The four-rows-per-workgroup form: a last workgroup with one row, both instantiations at 256 / 257 vectors, its widest d,
    and the width just past it; mixed value families, so that a row normalised with its neighbour's statistics (the next row's
    loads are in flight while this one reduces) is far outside the bound.  Bit-identical to the same rows in pieces of < 8192."""
    from magma_amd import ops
    x = kcmp.layernorm_family_rows("mixed", rows, d, seed=44)
    out, xv, g, b = run_layernorm(x, dev, "rows per workgroup, mixed rows")
    pieces = torch.cat([ops.layernorm(xv[i:i + 4096], g, b, EPS) for i in range(0, rows, 4096)])
    assert torch.equal(bits(out), bits(pieces))


@pytest.mark.parametrize("rows,d", [(5, 2056), (8193, 8)])
@pytest.mark.parametrize("kind", kcmp.LN_FAMILIES + ("mixed",))
def test_layernorm_value_families(dev, kind, rows, d):
    """Offset rows (cancellation in x - mean), constant rows (variance 0, rstd = eps^-1/2), one spike at column 0 / d - 1,
    all-zero rows, and all of them mixed in one call -- in the one-row and in the four-rows-per-workgroup form."""
    from magma_amd import ops
    out, xv, g, b = run_layernorm(kcmp.layernorm_family_rows(kind, rows, d, seed=60), dev, f"{kind} rows")
    if rows >= 8192:
        pieces = torch.cat([ops.layernorm(xv[i:i + 4096], g, b, EPS) for i in range(0, rows, 4096)])
        assert torch.equal(bits(out), bits(pieces))
    if kind == "zero":          # exactly beta, rounded
        assert torch.equal(bits(out), bits(b.to(BF16).expand(rows, d)))


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------------
def single_element_dy(rows, d):
    """Zero except one element per row (another column in every row): dx is then the two mean terms everywhere else."""
    dy = torch.zeros(rows, d)
    r = torch.arange(rows)
    dy[r, (r * 37 + d - 1) % d] = 1.5
    return dy.to(BF16)


@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("d", [8, 2040, 2048, 2056, 8184, 8192])
def test_layernorm_bwd_edges(dev, rows, d):
    """Every combination of res given or not and xhat wanted or not, on offset and one-spike x, with a dense dy and a dy of one
    element per row; dy, x and res each with another row stride, all inside NaN-filled parents."""
    from magma_amd import ops
    g = rnd(d, seed=9) * 0.1 + 1
    gp, gv, gs = framed_vec(g, NAN, dev)
    resp, res, ress = framed(rnd(rows, d, seed=8).to(BF16), d + 40, NAN, dev)
    for xkind in ("offset", "spike"):
        xp, x, xs = framed(kcmp.layernorm_family_rows(xkind, rows, d, seed=6), d + 24, NAN, dev)
        for dykind, dy_cpu in (("dense dy", rnd(rows, d, seed=7).to(BF16)), ("one-element dy", single_element_dy(rows, d))):
            dyp, dy, dys = framed(dy_cpu, d + 8, NAN, dev)
            for r in (res, None):
                what = f"layernorm_bwd {rows}x{d}, {xkind} x, {dykind}, res {r is not None}"
                R = kcmp.layernorm_bwd_reference(dy, x, gv, EPS, res=r)
                poison_allocator((rows, d), BF16, dev)
                dx, xh = ops.layernorm_bwd(dy, x, gv, EPS, res=r, want_xhat=True)
                assert dx.shape == xh.shape == (rows, d)
                kcmp.assert_elementwise(dx, *R["dx"], what + ": dx")
                kcmp.assert_elementwise(xh, *R["xhat"], what + ": xhat")
                poison_allocator((rows, d), BF16, dev)
                dx_only = ops.layernorm_bwd(dy, x, gv, EPS, res=r)
                assert torch.equal(bits(dx_only), bits(dx)), what + ": dx depends on whether xhat is written"
            assert_unchanged(dyp, dys, "layernorm_bwd dy")
        assert_unchanged(xp, xs, "layernorm_bwd x")
    assert_unchanged(resp, ress, "layernorm_bwd res")
    assert_unchanged(gp, gs, "layernorm_bwd gamma")


def test_layernorm_bwd_refuses_bad_operands(dev):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    z = lambda *s: torch.zeros(*s, dtype=BF16, device=dev)
    with pytest.raises(MagmaHipError):
        ops.layernorm_bwd(z(2, 8200), z(2, 8200), torch.ones(8200, device=dev))
    d = 64
    g = torch.ones(d, device=dev)
    with pytest.raises(AssertionError):
        ops.layernorm_bwd(z(2, d), z(2, d), g.to(BF16))                      # would be read as fp32
    with pytest.raises(AssertionError):
        ops.layernorm_bwd(z(2, d), z(2, d), torch.ones(d + 8, device=dev))
    with pytest.raises(AssertionError):
        ops.layernorm_bwd(z(2, d), z(2, d), g, res=z(2, d).float())
    with pytest.raises(AssertionError):
        ops.layernorm_bwd(z(2, d), z(2, d), g, res=z(3, d))
    with pytest.raises(AssertionError):
        ops.layernorm_bwd(z(2, d), z(2, d), g, res=z(2, 2 * d)[:, ::2])


# ---------------------------------------------------------------------------------------------------------------------------
# cross-entropy
# ---------------------------------------------------------------------------------------------------------------------------
PAD = 1e30          # what the pad columns [V, Vp) and the rows around the logits hold: read once, a sum is off by 30 orders


def stats_of(loss):
    """The [mean, valid count] pair the mean-loss scalar is element 0 of."""
    stats = loss._base
    assert stats is not None and stats.shape == (2,) and loss.data_ptr() == stats.data_ptr()
    return stats


def ce_direct(logits, tg, ld_out):
    """The three launches of ops.cross_entropy_fwd_bwd with outputs this test owns: NaN-filled, framed -> (rows, stats, dlogits)."""
    from magma_amd import lib as L
    dev = logits.device
    R, V = logits.shape
    s = torch.cuda.current_stream().cuda_stream
    rp, rows = framed_out(R, 1, 1, F32, dev)
    sp, stats = framed_out(1, 2, 2, F32, dev)
    dp, dl = framed_out(R, ld_out, ld_out, BF16, dev)
    lib = L.load()
    L.check(lib.mg_ce_rows_f32(logits.data_ptr(), logits.stride(0), tg.data_ptr(), rows.data_ptr(), R, V, s), "mg_ce_rows_f32")
    L.check(lib.mg_ce_reduce_f32(rows.data_ptr(), tg.data_ptr(), R, V, stats.data_ptr(), s), "mg_ce_reduce_f32")
    L.check(lib.mg_ce_bwd_bf16(logits.data_ptr(), logits.stride(0), tg.data_ptr(), stats.data_ptr(), dl.data_ptr(), ld_out, R, V, s),
            "mg_ce_bwd_bf16")
    assert_frame_untouched(rp, rows, NAN, "ce rows")
    assert_frame_untouched(sp, stats, NAN, "ce stats")
    assert_frame_untouched(dp, dl, NAN, "ce d logits")
    return rows.reshape(R), stats.reshape(2), dl


def run_cross_entropy(lg_cpu, tg_cpu, dev, ld_extra, what):
    """Both ops on logits = buf[:, :V] of a [.., Vp] buffer full of 1e30, per element against cross_entropy_reference; the ops'
    own outputs must equal, bit for bit, the ones written into NaN-filled memory (every element written, pad columns zero)."""
    from magma_amd import ops
    R, V = lg_cpu.shape
    Vp = ops.ceil_to(V, 8)
    ld_out = Vp + ld_extra
    bufp, logits, bufs = framed(lg_cpu, Vp, PAD, dev)
    tp, tg, ts = framed_vec(tg_cpu, 0, dev)
    C = kcmp.cross_entropy_reference(logits, tg)
    loss, rows = ops.cross_entropy(logits, tg)
    loss2, dl = ops.cross_entropy_fwd_bwd(logits, tg, ld_out)
    rows_d, stats_d, dl_d = ce_direct(logits, tg, ld_out)
    assert dl.shape == (R, ld_out) and dl.dtype == BF16 and rows.shape == (R,)
    assert torch.equal(bits(rows), bits(rows_d)) and torch.equal(bits(dl), bits(dl_d))
    for st in (stats_of(loss), stats_of(loss2)):
        assert torch.equal(bits(st), bits(stats_d))
        assert float(st[1]) == C["n_valid"], f"{what}: stats[1] = {float(st[1])}, {C['n_valid']} valid targets"
    kcmp.assert_elementwise(rows, *C["rows"], f"cross-entropy {what}: row losses")
    if C["n_valid"]:
        kcmp.assert_elementwise(loss.reshape(1), *C["mean"], f"cross-entropy {what}: mean loss")
    else:
        assert math.isnan(float(loss)) and math.isnan(float(loss2))
    kcmp.assert_elementwise(dl[:, :V], *C["dlogits"], f"cross-entropy {what}: d logits")
    assert bool((bits(dl[:, V:]) == 0).all()), f"{what}: columns [V, ld_out) of d logits are not +0"
    assert_unchanged(bufp, bufs, f"cross-entropy {what}: logits buffer")
    assert_unchanged(tp, ts, f"cross-entropy {what}: targets")
    return C, rows, dl


def check_family_exactness(kind, C, rows, dl, V, what):
    if kind == "peaked":
        assert bool((rows == 0).all()) and bool((dl == 0).all()), f"{what}: loss and gradient of a row whose target holds all the mass are 0"
    if kind == "ignored":
        assert C["n_valid"] == 0 and bool((rows == 0).all()) and bool((bits(dl) == 0).all())
    if kind == "peaked off" and V > 1:
        n = C["n_valid"]
        ref = C["dlogits"][0]
        assert bool(((ref != 0).sum(1) == 2).all()) and float(ref.max()) == 1.0 / n and float(ref.min()) == -1.0 / n


@pytest.mark.parametrize("ld_extra", [0, 56])
@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 1053])
def test_cross_entropy_vocabulary_edges(dev, V, ld_extra):
    for kind in kcmp.CE_FAMILIES:
        lg, tg = kcmp.cross_entropy_family(kind, 5, V, seed=111)
        what = f"{kind} R=5 V={V} ld_out=Vp+{ld_extra}"
        C, rows, dl = run_cross_entropy(lg, tg, dev, ld_extra, what)
        check_family_exactness(kind, C, rows, dl, V, what)


@pytest.mark.parametrize("ld_extra", [0, 56])
def test_cross_entropy_full_vocabulary(dev, ld_extra):
    """V = 50258 inside Vp = 50264: 196 passes of the 256-thread loops and a tail of 82."""
    V = 50258
    for kind in kcmp.CE_FAMILIES:
        lg, tg = kcmp.cross_entropy_family(kind, 3, V, seed=112)
        what = f"{kind} R=3 V={V} ld_out=Vp+{ld_extra}"
        C, rows, dl = run_cross_entropy(lg, tg, dev, ld_extra, what)
        check_family_exactness(kind, C, rows, dl, V, what)


@pytest.mark.parametrize("R", [1, 255, 256, 257, 4099])
def test_cross_entropy_row_count_edges(dev, R):
    """The reduction's 256-thread loop over the rows and its count, about a quarter of the targets ignored."""
    V = 64
    lg, tg = kcmp.cross_entropy_family("gauss", R, V, seed=113)
    drop = torch.rand(R, generator=torch.Generator().manual_seed(R)) < 0.25
    if R > 1:
        drop[0] = False
    tg[drop] = -100
    C, rows, dl = run_cross_entropy(lg, tg, dev, 0, f"gauss R={R} V={V}")
    assert C["n_valid"] == int((~drop).sum())


def test_cross_entropy_targets_outside_the_vocabulary_are_ignored(dev):
    """A target >= V or negative is ignored by all three kernels alike: loss 0, gradient 0, NOT counted.  (Before mg_ce_reduce_f32
    knew V it counted every target >= 0: here 4 instead of 2, half the mean loss and half of every gradient.)"""
    V = 257
    lg, _ = kcmp.cross_entropy_family("gauss", 6, V, seed=114)
    tg = torch.tensor([3, 256, 257, 10 ** 6, -1, -100], dtype=I64)
    for ld_extra in (0, 56):
        C, rows, dl = run_cross_entropy(lg, tg, dev, ld_extra, f"targets outside [0, {V})")
        assert C["n_valid"] == 2
        assert bool((rows[2:] == 0).all()) and bool((bits(dl[2:]) == 0).all())
        sm = torch.softmax(lg[:2].double(), -1)
        sm[0, 3] -= 1.0
        sm[1, 256] -= 1.0
        assert torch.allclose(C["dlogits"][0][:2].cpu(), sm / 2, rtol=1e-12, atol=1e-300)
        mean2 = torch.nn.functional.cross_entropy(lg[:2].double(), tg[:2])
        assert torch.allclose(C["mean"][0].cpu(), mean2.reshape(1), rtol=1e-12)


def test_both_engines_refuse_a_label_outside_the_head(dev):
    """A caption id >= V: the training step (labels on the host, MagmaEngine.forward_train) and the evaluation loss
    (LMEngine.forward_loss) raise ValueError naming the id and V instead of returning a loss over fewer rows."""
    from magma_amd.testing import build_reduced_magma
    from magma_amd.train_engine import MagmaEngine
    model = build_reduced_magma(dev, n_positions=128)
    V, S = model.lm.engine.V, model.seq_len
    g = torch.Generator().manual_seed(4)
    images = torch.randn(2, 3, 64, 64, generator=g)
    caps = torch.full((2, S), model.eos_token, dtype=I64)
    caps[0, :23] = torch.randint(0, 1000, (23,), generator=g)
    caps[1, :11] = torch.randint(0, 1000, (11,), generator=g)
    bad = caps.clone()
    bad[1, 4] = V
    eng = MagmaEngine(model)
    for mode in (eng.train, eng.eval):
        mode()
        assert math.isfinite(float(eng(images, caps).loss))
        with pytest.raises(ValueError, match=rf"label id {V} .*V = {V}\b"):
            float(eng(images, bad).loss)
    behind = caps.clone()
    behind[1, 20] = V                          # behind the first eos: masked by build_labels, never a label
    for mode in (eng.train, eng.eval):
        mode()
        assert math.isfinite(float(eng(images, behind).loss))


def test_cross_entropy_refuses_bad_operands(dev):
    from magma_amd import ops
    lg = torch.zeros(4, 16, device=dev)
    tg = torch.zeros(4, dtype=I64, device=dev)
    for bad_lg, bad_tg, ld in ((lg.to(BF16), tg, 16), (lg, tg.int(), 16), (lg, tg[:3], 16), (lg, tg, 8), (lg.t(), tg, 16)):
        with pytest.raises(AssertionError):
            ops.cross_entropy_fwd_bwd(bad_lg, bad_tg, ld)
    with pytest.raises(AssertionError):
        ops.cross_entropy(lg.to(BF16), tg)


# ---------------------------------------------------------------------------------------------------------------------------
# argmax
# ---------------------------------------------------------------------------------------------------------------------------
def argmax_rows(V, seed):
    """Rows of N(0, 1) (all below 50) with maxima of 100 placed where the kernel changes hands.  A row base that is 16-byte aligned
    is read as float4s, thread t taking quads t, t + 1024, t + 2048, t + 3072 of each 4096-quad pass (four loads in flight) and the
    last V % 4 elements by a scalar loop; another row base is read by the scalar loop alone.  -> fp32 [B, V] on the CPU."""
    NEG = float("-inf")
    tail0 = (V >> 2) << 2
    singles = {0, V - 1, tail0, tail0 - 1, 255, 256, 4095, 4096, 4097}        # ends, scalar tail, wave 0 | 1, thread 1023 | 0
    for u in (1, 2, 3):
        singles |= {4 * 1024 * u - 1, 4 * 1024 * u, 4 * 1024 * u + 1}           # edges of the four loads in flight
    singles |= {16384 - 1, 16384, 16384 + 1, 16384 + 4}                        # the second pass of the 4096-quad loop
    ties = [(5, 6),                       # inside one 16-byte load
            (8, 8 + 4096),                # quads 2 and 1026: two of one thread's loads in flight
            (8 + 4096 * 3, 8 + 16384),    # one thread, two passes
            (40, 400),                    # threads 10 and 100: waves 0 and 1
            (3 * 256 + 2, 15 * 256 + 1),  # waves 3 and 15
            (17, V - 1),                  # vector part and scalar tail (V % 4 != 0)
            (tail0, V - 1)]               # both in the tail
    rows = []
    g = torch.Generator().manual_seed(seed)
    def base():
        return torch.randn(V, generator=g).clamp_(-40, 40)
    for p in sorted(i for i in singles if 0 <= i < V):
        r = base(); r[p] = 100.0; rows.append(r)
    for a, b in ties:
        if 0 <= a < b < V:
            r = base(); r[a] = r[b] = 100.0; rows.append(r)
    rows.append(torch.full((V,), NEG))                                             # nothing is larger than -inf: index 0
    for p in sorted({0, V // 2, V - 1}):
        r = torch.full((V,), NEG); r[p] = -3.0e38; rows.append(r)                  # logits processors ban with -inf
    r = base(); r[: V // 2] = NEG; rows.append(r)
    return torch.stack(rows)


@pytest.mark.parametrize("V", [1, 3, 4, 5, 1023, 1024, 1025, 4096, 4097, 16384 + 5, 50258])
def test_argmax_edges(dev, V):
    """Exact against torch.argmax on the CPU (first maximum wins), on views buf[:, :V] whose pad columns hold +inf; row strides
    that leave every row base 16-byte aligned, and strides that leave only some of them aligned."""
    from magma_amd import ops
    lg = argmax_rows(V, seed=91)
    B = lg.shape[0]
    ref = torch.argmax(lg, dim=-1)
    lds = [V + 3, ops.ceil_to(V, 4) + 4] + ([V + 6] if V % 2 == 0 else [])
    for ld in lds:
        bufp, view, bufs = framed(lg, ld, float("inf"), dev)
        tokp, tok = framed_out(B, 1, 1, I64, dev, fill=-7)
        tok = tok.reshape(B)
        ret = ops.argmax(view, out=tok)
        assert ret is tok
        got = tok.cpu()
        wrong = (got != ref).nonzero().flatten().tolist()
        assert not wrong, f"argmax V={V} ld={ld}: rows {wrong[:8]} give {got[wrong[:8]].tolist()}, torch.argmax {ref[wrong[:8]].tolist()}"
        assert_frame_untouched(tokp, tok.reshape(B, 1), -7, f"argmax V={V} tokens")
        assert_unchanged(bufp, bufs, f"argmax V={V} logits")
    assert torch.equal(ops.argmax(view).cpu(), ref)


# ---------------------------------------------------------------------------------------------------------------------------
# embedding gather
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(1, 1), (3, 7)])
@pytest.mark.parametrize("d", [8, 2040, 2048, 2056, 4096])
def test_embedding_edges(dev, d, B, T):
    """Rows of 1, 255, 256, 257 and 512 vectors (the copy loop steps by 256), first and last id, repeated ids, and the clamp: ids
    below 0 read row 0, ids >= vocab read row vocab - 1 -- never the trap rows that surround the table."""
    from magma_amd import ops
    vocab, extra, TRAP, SENT = 11, 5, -3.0e38, 77.0
    wp, wte, ws = framed(rnd(vocab, d, seed=51).to(BF16), d, TRAP, dev)
    assert wte.is_contiguous()
    pool = [0, vocab - 1, 5, 5, 5, -1, -10 ** 12, vocab, 2 ** 40, 2 ** 31, -2 ** 31, 3, vocab - 1, 0, 7, 2 ** 63 - 1, -2 ** 63, 1, 9, 2, 5]
    S_total = T + extra
    for row_off in (0, S_total - T):
        for start in ((0, 1, 5, 6, 7, 8) if B * T == 1 else (0,)):
            ids_cpu = torch.tensor([pool[(start + i) % len(pool)] for i in range(B * T)], dtype=I64).reshape(B, T)
            ids = ids_cpu.to(dev)
            outp = torch.full((B + 2, S_total, d), SENT, dtype=BF16, device=dev)
            out = outp[1:1 + B]
            ops.embedding(ids, wte, out, row_off=row_off)
            want = torch.full_like(outp, SENT)
            want[1:1 + B, row_off:row_off + T] = wte[ids_cpu.clamp(0, vocab - 1).to(dev)]
            assert torch.equal(bits(outp), bits(want)), f"embedding d={d} B={B} T={T} row_off={row_off} ids {ids_cpu.flatten().tolist()}"
            assert not bool((outp == wp[0, 0]).any()), "a trap row of the table's parent reached the output"
    assert_unchanged(wp, ws, "embedding table")


# ---------------------------------------------------------------------------------------------------------------------------
# build_labels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 255, 256, 257, 700])
def test_build_labels_edges(dev, S):
    """Bit-exact against the oracle's restatement of the reference rule: the first eos among the T = S - P kept caption tokens at
    the ends of a thread's, a wave's and a pass's share of the row, with a second eos in another thread / wave / pass, with an eos
    only in the truncated tail [T, S), and with none; nine rows per call, P = 0, 1, S - 1, S."""
    from magma_amd import ops
    from oracle.model import build_labels
    eos, B = 1054, 9
    g = torch.Generator().manual_seed(7)
    for P in sorted({0, 1, S - 1, S}):
        T = S - P
        firsts = sorted({t for t in (0, 63, 64, 255, 256, 257, T - 1) if 0 <= t < T})
        plans = [[]]                                                            # no eos at all
        if P > 0:
            plans += [[T], [S - 1]]                                             # only inside the truncated tail
        for t in firsts:
            plans.append([t])
            plans += [[t, t2] for t2 in (t + 1, t + 64, t + 256, T - 1, S - 1) if t < t2 < S]
        while len(plans) % B:
            plans.append([])
        for i in range(0, len(plans), B):
            cap = torch.randint(0, 1000, (B, S), generator=g)
            for r, plan in enumerate(plans[i:i + B]):
                for t in plan:
                    cap[r, t] = eos
            got = ops.build_labels(cap.to(dev), P, eos).cpu()
            ref = build_labels(P, cap, eos)
            assert torch.equal(got, ref), f"build_labels S={S} P={P}: rows {(got != ref).any(1).nonzero().flatten().tolist()} of plans {plans[i:i + B]}"
