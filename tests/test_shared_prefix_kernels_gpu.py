"""Decode attention over one shared session prefix (DESIGN.md "Shared session prefix"), the kernels alone: the prefix-partials launch
(ops.attn_decode_prefix) followed by the shared mode of the fused decode attention (ops.attn_decode_fused / ops.decode_attn_gemv with
``shared=``), per element against the fp64 attention over the concatenation [prefix; own] -- and the existing fused kernel on caches
that hold the prefix copied in, against the same reference with the same inputs --, the exact properties (a row's bits do not depend
on the other rows, the appended k / v are the existing kernel's, nothing else is written, a position below P is P), the admission
launch with a destination offset against an indexed copy, and every refusal of the new entry points.

NaN bit patterns fill everything a kernel must not read: the prefix buffer beyond P, every own cache beyond the row's length, the qkv
rows >= B, and guard bands around every buffer a kernel writes."""
import ctypes as C

import pytest
import torch

import kernel_compare as kcmp
from device_indices import Guarded
from test_stream_kernels_gpu import EOS_IDS, FILL, HC, SEQS, _session_state
from test_stream_prefix_kernels_gpu import BOOK, REQS, _caches, admit_at, eq16, first_code

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
H, DH, D = 2, 256, 512
CHUNK = 64                      # ops.PREFIX_CHUNK (asserted below)
SMAX_OWN = 128
NAN16 = 0x7FC1                  # a quiet bf16 NaN with a payload
GUARD = 4096                    # elements of NaN pattern on each side of a guarded buffer
PS = [1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
OWN_LENS = [1, 2, 17, 64]
FAMILIES = ("random", "dominant in the prefix", "dominant in the own part", "one chunk underflows", "chunk edges")


def rnd(*shape, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def tables(rot, n, dev):
    from oracle.model import rotary_tables
    if rot == 0:
        z = torch.zeros(n, 1, dtype=torch.float32, device=dev)
        return z, z.clone()
    s, c = rotary_tables(rot, n)
    return s.to(dev).contiguous(), c.to(dev).contiguous()


def own_lens_of(B, P):
    """Ragged own lengths (the appended token included): every length of OWN_LENS appears over the rows and the values of P."""
    shift = PS.index(P) if P in PS else 0
    return [OWN_LENS[(b + shift) % 4] for b in range(B)]


def build(dev, B, P, rot, family, seed=0, lens=None):
    """One case.  Returns a dict: qkv16 [16, 3 D] (rows >= B NaN), kpre / vpre Guarded [H, Spre, 256] (NaN beyond P), kown / vown
    Guarded [B, H, SMAX_OWN, 256] (NaN from own index len - 1 on: the kernel appends there), d_pos [B] = P + len - 1, the full caches
    kfull / vfull [B, H, P + SMAX_OWN, 256] for the existing kernel (the prefix copied in), q_rot [B, H, 1, 256]."""
    from magma_amd import ops
    lens = own_lens_of(B, P) if lens is None else lens
    Spre = -(-P // 64) * 64 + 64
    Sfull = -(-(P + SMAX_OWN) // 64) * 64
    sin_t, cos_t = tables(rot, Sfull, dev)
    qkv16 = torch.empty(16, 3 * D, dtype=BF16, device=dev)
    Guarded.fill_nan(qkv16)
    qkv16[:B] = rnd(B, 3 * D, dev=dev, seed=seed + 1, scale=0.5).to(BF16)
    pre_k = rnd(H, P, DH, dev=dev, seed=seed + 2, scale=0.5).to(BF16)
    pre_v = rnd(H, P, DH, dev=dev, seed=seed + 3).to(BF16)
    own_k = rnd(B, H, SMAX_OWN, DH, dev=dev, seed=seed + 4, scale=0.5).to(BF16)
    own_v = rnd(B, H, SMAX_OWN, DH, dev=dev, seed=seed + 5).to(BF16)
    d_pos = torch.tensor([P + n - 1 for n in lens], dtype=torch.int32, device=dev)
    if family == "dominant in the own part":            # k of the new token = 2 q: the rotary turns both by the same angle
        qkv16[:B, D:2 * D] = (qkv16[:B, :D].float() * 2).to(BF16)
    if family == "one chunk underflows":
        # dim 255 is not rotated (rot <= 64): every q carries 16 there, the keys of chunk 0 carry -200, all other keys 0 -- the scores
        # of chunk 0 lie 200 units below the rest (with P <= CHUNK: the whole prefix below the own part)
        qkv16[:B].view(B, 3, H, DH)[:, 0, :, 255] = 16.0
        qkv16[:B].view(B, 3, H, DH)[:, 1, :, 255] = 0.0
        pre_k[:, :, 255] = 0.0
        own_k[:, :, :, 255] = 0.0
        pre_k[:, :CHUNK, 255] = -200.0
    # the rotated q of every row (the existing rotary launch, which the fused kernels equal bit for bit: test_kernels_gpu)
    q_rot = torch.empty(B, H, 1, DH, dtype=BF16, device=dev)
    ksink, vsink = torch.empty(B, H, Sfull, DH, dtype=BF16, device=dev), torch.empty(B, H, Sfull, DH, dtype=BF16, device=dev)
    if rot:
        ops.rotary_split(qkv16[:B], B, 1, H, rot, sin_t, cos_t, q_rot, ksink, vsink, d_pos=d_pos, pos_stride=1)
    else:
        q_rot.copy_(qkv16[:B, :D].reshape(B, H, 1, DH))
    if family == "dominant in the prefix":              # the middle key of the prefix = 2 q of row 0
        pre_k[:, P // 2] = (q_rot[0, :, 0].float() * 2).to(BF16)
    if family == "chunk edges":                         # first and last key of every chunk and key P - 1 = 4 q of row (key mod B)
        qsel = torch.stack([q_rot[j % B, :, 0] for j in range(P)], 1)
        pre_k = kcmp.dominant_edge_keys(qsel, pre_k, tile=CHUNK)
    kpre, vpre = Guarded((H, Spre, DH), BF16, dev), Guarded((H, Spre, DH), BF16, dev)
    kpre.t[:, :P], vpre.t[:, :P] = pre_k, pre_v
    kown, vown = Guarded((B, H, SMAX_OWN, DH), BF16, dev), Guarded((B, H, SMAX_OWN, DH), BF16, dev)
    kfull = torch.empty(B, H, Sfull, DH, dtype=BF16, device=dev)
    vfull = torch.empty(B, H, Sfull, DH, dtype=BF16, device=dev)
    Guarded.fill_nan(kfull)
    Guarded.fill_nan(vfull)
    kfull[:, :, :P], vfull[:, :, :P] = pre_k, pre_v
    for b, n in enumerate(lens):
        kown.t[b, :, :n - 1], vown.t[b, :, :n - 1] = own_k[b, :, :n - 1], own_v[b, :, :n - 1]
        kfull[b, :, P:P + n - 1], vfull[b, :, P:P + n - 1] = own_k[b, :, :n - 1], own_v[b, :, :n - 1]
    return dict(B=B, P=P, rot=rot, lens=lens, qkv16=qkv16, kpre=kpre, vpre=vpre, kown=kown, vown=vown, d_pos=d_pos, kfull=kfull,
                vfull=vfull, q_rot=q_rot, sin_t=sin_t, cos_t=cos_t, part=Guarded((B, H, -(-P // CHUNK), 264), torch.float32, dev))


def run_shared(c, gemv=None, d_pos=None):
    """Kernel 1 then kernel 2 on the case's own buffers -> out [B, D] (rows of a NaN-filled guarded buffer)."""
    from magma_amd import ops
    B, P = c["B"], c["P"]
    d_pos = c["d_pos"] if d_pos is None else d_pos
    out = Guarded((B, D), BF16, c["qkv16"].device)
    ops.attn_decode_prefix(c["qkv16"], c["kpre"].t, c["vpre"].t, c["part"].t, B, H, P, d_pos, c["rot"], c["sin_t"], c["cos_t"])
    kw = dict(pos_stride=1, shared=(P, c["part"].t))
    if gemv is None:
        ops.attn_decode_fused(c["qkv16"], c["kown"].t, c["vown"].t, out.t, B, H, d_pos, c["rot"], c["sin_t"], c["cos_t"], **kw)
    else:
        ops.decode_attn_gemv(c["qkv16"], c["kown"].t, c["vown"].t, out.t, B, H, d_pos, c["rot"], c["sin_t"], c["cos_t"], gemv, **kw)
    assert out.guards_intact()
    return out.t


def merge_ops(n_chunk):
    """NAMED term: fp32 roundings the merge adds on the way of a term -- per chunk and for the own part one multiply by its weight
    and one addition, in numerator and denominator alike, and the final division."""
    return 2 * (n_chunk + 1) + 2


def assert_against_fp64(c, out, what, merged):
    """Per element against fp64 softmax(q [prefix; own]^T / 16) [prefix; own] of every row, the appended token included."""
    P, worst = c["P"], 0.0
    n_chunk = -(-P // CHUNK)
    for b, n in enumerate(c["lens"]):
        ctx = P + n
        T = kcmp.attention_terms(c["q_rot"][b], c["kfull"][b, :, :ctx], c["vfull"][b, :, :ctx])
        n_fp32 = ctx + ctx / 16 + 16 + (merge_ops(n_chunk) if merged else 0)
        bound = kcmp.attention_bound(T, ctx, out.dtype, p_dtype=torch.float32, n_rescale=n_chunk + 1 if merged else 0, n_fp32=n_fp32)
        worst = max(worst, kcmp.assert_elementwise(out[b].view(H, 1, DH), T["ref"], bound, f"{what}, row {b} (P {P} + own {n})"))
    return worst


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("B", [1, 3, 16])
def test_shared_attention_against_fp64_and_beside_the_existing_kernel(dev, B, P):
    from magma_amd import ops
    assert (ops.PREFIX_CHUNK, ops.PREFIX_PART) == (CHUNK, 264) and ops.prefix_chunks(P) == -(-P // CHUNK)
    for rot in (0, 64):
        for fi, family in enumerate(FAMILIES):
            c = build(dev, B, P, rot, family, seed=100 * fi + rot)
            snap = [g.t.view(torch.int16).clone() for g in (c["kpre"], c["vpre"], c["kown"], c["vown"])]
            tag = f"B {B} P {P} rot {rot} {family}"
            # the existing kernel on the caches that hold the prefix copied in: appends, and is the other path under the same bound
            old = torch.empty(B, D, dtype=BF16, device=dev)
            ops.attn_decode_fused(c["qkv16"], c["kfull"], c["vfull"], old, B, H, c["d_pos"], rot, c["sin_t"], c["cos_t"], pos_stride=1)
            out = run_shared(c)
            assert not bool(out.isnan().any()) and not bool(old.isnan().any()), tag
            w_new = assert_against_fp64(c, out, f"shared prefix, {tag}", merged=True)
            w_old = assert_against_fp64(c, old, f"existing fused kernel, {tag}", merged=False)
            print(f"{tag}: worst error / bound {w_new:.3f} shared, {w_old:.3f} existing")
            # the appended k, v are the existing kernel's at the shifted index, nothing else was written, the prefix is untouched
            for own, full, before in ((c["kown"], c["kfull"], snap[2]), (c["vown"], c["vfull"], snap[3])):
                want = before.clone()
                for b, n in enumerate(c["lens"]):
                    want[b, :, n - 1] = full[b, :, P + n - 1].view(torch.int16)
                    assert not bool(full[b, :, P + n - 1].isnan().any())
                assert torch.equal(own.t.view(torch.int16), want), tag
                assert own.guards_intact()
            assert torch.equal(c["kpre"].t.view(torch.int16), snap[0]) and torch.equal(c["vpre"].t.view(torch.int16), snap[1])
            assert c["kpre"].guards_intact() and c["vpre"].guards_intact() and c["part"].guards_intact()
            if family == "one chunk underflows":        # the precondition: chunk 0's weight is 0 in fp32, and it is a partial
                m = c["part"].t[:, :, :, 256]
                own_or_rest = torch.full_like(m[:, :, 0], -1e30) if m.shape[2] == 1 else m[:, :, 1:].max(-1).values
                assert bool((m[:, :, 0] < -150).all()) and (m.shape[2] == 1 or bool((own_or_rest - m[:, :, 0] > 150).all())), tag


def test_colaunch_with_a_gemv_is_the_standalone_launch(dev):
    """ops.decode_attn_gemv(shared=) writes the bits of ops.attn_decode_fused(shared=) -- also into a wider row --, and its GEMV is right."""
    from magma_amd import ops
    B, P = 3, 2 * CHUNK + 1
    a, b = build(dev, B, P, 64, "random", seed=7), build(dev, B, P, 64, "random", seed=7)
    x = rnd(B, 512, dev=dev, seed=84).to(BF16)
    w = rnd(264, 512, dev=dev, seed=85, scale=0.05).to(BF16)
    lin = ops.PackedLinear(w, bias=rnd(264, dev=dev, seed=86))
    y = torch.empty(B, 264, dtype=torch.float32, device=dev)
    alone = run_shared(a)
    beside = run_shared(b, gemv=(x, lin, y, {"out_dtype": torch.float32}))
    assert eq16(alone, beside) and eq16(a["kown"].t, b["kown"].t) and eq16(a["vown"].t, b["vown"].t)
    kcmp.assert_linear(y, "decode_attn_gemv(shared=), the co-launched GEMV", x, w, bias=lin.bias)
    wide = torch.zeros(B, D + 64, dtype=BF16, device=dev)
    c = build(dev, B, P, 64, "random", seed=7)
    ops.attn_decode_prefix(c["qkv16"], c["kpre"].t, c["vpre"].t, c["part"].t, B, H, P, c["d_pos"], 64, c["sin_t"], c["cos_t"])
    ops.decode_attn_gemv(c["qkv16"], c["kown"].t, c["vown"].t, wide[:, :D], B, H, c["d_pos"], 64, c["sin_t"], c["cos_t"],
                         (x, lin, y, {"out_dtype": torch.float32}), pos_stride=1, shared=(P, c["part"].t))
    assert eq16(wide[:, :D].contiguous(), alone) and not bool(wide[:, D:].any())


def rows_case(c, rows, dev):
    """The case restricted to (and ordered as) ``rows``: fresh buffers that hold the same bits."""
    n = len(rows)
    r = dict(c, B=n, lens=[c["lens"][i] for i in rows], d_pos=c["d_pos"][rows].contiguous())
    qkv16 = torch.empty_like(c["qkv16"])
    Guarded.fill_nan(qkv16)
    qkv16[:n] = c["qkv16"][rows]
    r["qkv16"] = qkv16
    for name in ("kown", "vown"):
        g = Guarded((n, H, SMAX_OWN, DH), BF16, dev)
        g.t.copy_(c[name].t[rows])
        r[name] = g
    r["part"] = Guarded((n, H, -(-c["P"] // CHUNK), 264), torch.float32, dev)
    return r


def test_a_row_does_not_depend_on_the_other_rows(dev):
    """Row b's context row, as int16: alone (B = 1), among 16 rows, and under a permutation of the rows."""
    B, P = 16, 2 * CHUNK + 1
    c = build(dev, B, P, 64, "random", seed=11)
    pristine = rows_case(c, list(range(B)), dev)        # build()'s buffers before any launch
    out = run_shared(c).clone()
    assert len({tuple(out[b].view(torch.int16).tolist()) for b in range(B)}) == B
    for b in (0, 5, 15):
        alone = run_shared(rows_case(pristine, [b], dev))
        assert eq16(alone[0], out[b]), b
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(B, generator=g).tolist()
    assert perm != list(range(B))
    permuted = run_shared(rows_case(pristine, perm, dev))
    for r, b in enumerate(perm):
        assert eq16(permuted[r], out[b]), (r, b)
    few = run_shared(rows_case(pristine, [15, 2, 9], dev))
    assert eq16(few[0], out[15]) and eq16(few[1], out[2]) and eq16(few[2], out[9])


@pytest.mark.parametrize("P", [1, CHUNK + 1])
def test_a_position_below_the_prefix_counts_as_the_prefix(dev, P):
    """d_pos < P (an idle slot before its first occupant): the row appends at own index 0 and attends over the prefix and that one
    key, exactly as at d_pos = P; guard bands of NaN around the own caches, the prefix and the partials stay intact."""
    B = 3
    ref = build(dev, B, P, 64, "random", seed=13, lens=[1, 1, 1])
    want = run_shared(ref).clone()
    for low in ([0, 0, 0], [P - 1, 0, P // 2]):
        c = build(dev, B, P, 64, "random", seed=13, lens=[1, 1, 1])
        out = run_shared(c, d_pos=torch.tensor(low, dtype=torch.int32, device=dev))
        assert eq16(out, want), low
        for name in ("kown", "vown", "kpre", "vpre", "part"):
            assert c[name].guards_intact(), name
            if name != "part":
                assert eq16(c[name].t, ref[name].t), name


# ------------------------------------------------------------------------------------------------------------ admission
L_, N_STAGE, S_STAGE, B_, SMAX = 2, 5, 128, 5, 192


def admit_shared(ks, vs, kc, vc, src, dst, lens, first, limits, st, table, pos0, dst0):
    """The new entry point itself."""
    from magma_amd import lib
    n = len(src)
    arr = lambda xs: (C.c_int32 * max(n, 1))(*[int(x) for x in xs])  # noqa: E731
    h = st["history"]
    lib.check(lib.load().mg_slots_admit_shared_bf16(
        ks.data_ptr(), vs.data_ptr(), ks.shape[1], ks.shape[3], kc.data_ptr(), vc.data_ptr(), ks.shape[0], kc.shape[1], ks.shape[2],
        kc.shape[3], n, arr(src), arr(dst), arr(lens), first.data_ptr(), arr(limits), st["state"].data_ptr(), st["d_pos"].data_ptr(),
        st["token"].data_ptr(), st["finish"].data_ptr(), st["slot"].data_ptr(), h.data_ptr(), h.stride(0), h.shape[1], table.data_ptr(),
        len(EOS_IDS), len(SEQS), int(pos0), int(dst0), torch.cuda.current_stream().cuda_stream), "mg_slots_admit_shared_bf16")


@pytest.fixture(scope="module")
def caches(dev):
    """(kstage, vstage, kcache, vcache) of random bit patterns: made once, only ever cloned."""
    return _caches(dev, 3)


@pytest.mark.parametrize("dst0", [0, 5])
@pytest.mark.parametrize("P", [1, 31, 64])
def test_admit_shared_equals_indexed_copy(dev, caches, P, dst0):
    from magma_amd import ops
    ks, vs, kc0, vc0 = caches
    table = ops.stop_table(EOS_IDS, SEQS).to(dev)
    all_lens = [1, 7, 64, S_STAGE - P]
    n = 5
    reqs = REQS[:n]
    first = torch.tensor([r[2] for r in reqs], dtype=torch.int64, device=dev)
    for turn in range(4):                   # every request takes every length once
        lens = [all_lens[(j + turn) % 4] for j in range(n)]
        kc, vc, st = kc0.clone(), vc0.clone(), _session_state(dev, B_)
        want_k, want_v, want = kc0.clone(), vc0.clone(), {k: v.clone() for k, v in st.items()}
        args = (ks, vs, kc, vc, [r[0] for r in reqs], [r[1] for r in reqs], lens, first, [r[3] for r in reqs])
        if turn % 2:                        # through ops.slots_admit as the session calls it
            ops.slots_admit(*args, *[st[k] for k in BOOK], table, len(EOS_IDS), len(SEQS), pos0=P, dst0=dst0)
        else:
            admit_shared(*args, st, table, P, dst0)
        prev = 37
        c = prev % HC
        for (src, dst, t, limit), m in zip(reqs, lens):
            want_k[:, dst, :, dst0:dst0 + m] = ks[:, src, :, P:P + m]
            want_v[:, dst, :, dst0:dst0 + m] = vs[:, src, :, P:P + m]
            code = first_code(t, limit)
            want["d_pos"][dst], want["token"][dst] = P + m, t
            want["slot"][dst] = torch.tensor([c, limit], dtype=torch.int32)
            want["history"][dst, c] = t
            want["finish"][dst] = torch.tensor([-1, 0] if code is None else [prev, code], dtype=torch.int32)
        want["state"][1] = -1
        assert eq16(kc, want_k) and eq16(vc, want_v), (P, dst0, lens)
        assert not eq16(kc, kc0) and not eq16(vc, vc0)
        for name in BOOK:
            assert torch.equal(st[name], want[name]), (name, P, lens, st[name], want[name])
        # equal offsets: the bytes and the bookkeeping of mg_slots_admit_at_bf16
        k1, v1, s1 = kc0.clone(), vc0.clone(), _session_state(dev, B_)
        k2, v2, s2 = kc0.clone(), vc0.clone(), _session_state(dev, B_)
        short = [min(m, S_STAGE - P) for m in lens]
        admit_shared(ks, vs, k1, v1, *args[4:6], short, *args[7:], s1, table, P, P)
        admit_at(ks, vs, k2, v2, *args[4:6], short, *args[7:], s2, table, P)
        assert eq16(k1, k2) and eq16(v1, v2) and all(torch.equal(s1[k], s2[k]) for k in BOOK)


def test_admit_shared_refusals(dev, caches):
    from magma_amd.lib import MagmaHipError
    ks, vs, kc0, vc0 = caches
    from magma_amd import ops
    table = ops.stop_table(EOS_IDS, SEQS).to(dev)
    first = torch.full((8,), FILL, dtype=torch.int64, device=dev)

    def refused(kst, vst, kca, vca, lens, pos0, dst0):
        kca, vca = kca.clone(), vca.clone()
        st = _session_state(dev, kca.shape[1])
        keep = [t.clone() for t in (kca, vca, *st.values())]
        src, dst = list(range(len(lens))), list(range(len(lens)))[::-1]
        with pytest.raises(MagmaHipError, match="mg_slots_admit_shared_bf16"):
            admit_shared(kst, vst, kca, vca, src, dst, lens, first, [4] * len(lens), st, table, pos0, dst0)
        assert all(eq16(a, b) if a.dtype == BF16 else torch.equal(a, b) for a, b in zip(keep, (kca, vca, *st.values())))

    refused(ks, vs, kc0, vc0, [3], -1, 0)                                 # pos0 < 0
    refused(ks, vs, kc0, vc0, [3], 5, -1)                                 # dst0 < 0
    refused(ks, vs, kc0, vc0, [3, 0], 5, 0)                               # len < 1
    refused(ks, vs, kc0, vc0, [3, S_STAGE - 31 + 1], 31, 0)               # pos0 + len > S_stage: the source's own extent
    refused(ks, vs, kc0, vc0, [3, SMAX - 100 + 1], 1, 100)                # dst0 + len > Smax: the destination's own extent
    refused(ks, vs, kc0, vc0, [1], S_STAGE, 0)                            # no staged position behind pos0
    refused(ks, vs, kc0, vc0, [1], 0, SMAX)                               # no live position behind dst0
    refused(ks, vs, kc0, vc0, [1], 2 ** 31 - 1, 0)                        # nothing wraps
    refused(ks, vs, kc0, vc0, [1], 0, 2 ** 31 - 1)
    kc, vc, st = kc0.clone(), vc0.clone(), _session_state(dev, B_)
    admit_shared(ks, vs, kc, vc, [0], [0], [S_STAGE - 31], first, [4], st, table, 31, SMAX - (S_STAGE - 31))   # both bounds themselves pass
    assert int(st["d_pos"][0]) == S_STAGE and eq16(kc[:, 0, :, SMAX - (S_STAGE - 31):], ks[:, 0, :, 31:])


# ------------------------------------------------------------------------------------------------------------ refusals
def test_attention_refusals(dev):
    """Every refusal of the three attention entry points returns its error before any launch: the outputs keep their NaN fill."""
    from magma_amd import lib, ops
    from magma_amd.lib import MagmaHipError
    B, P = 3, 17
    c = build(dev, B, P, 64, "random", seed=17)
    out = Guarded((B, D), BF16, dev)
    x = rnd(B, 512, dev=dev, seed=84).to(BF16)
    lin = ops.PackedLinear(rnd(264, 512, dev=dev, seed=85, scale=0.05).to(BF16))
    y = torch.full((B, 264), float("nan"), dtype=torch.float32, device=dev)
    desc, _ = ops.skinny_desc(x, lin, y, out_dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    base = dict(qkv=c["qkv16"].data_ptr(), kpre=c["kpre"].t.data_ptr(), vpre=c["vpre"].t.data_ptr(), part=c["part"].t.data_ptr(),
                kown=c["kown"].t.data_ptr(), vown=c["vown"].t.data_ptr(), out=out.t.data_ptr(), B=B, H=H, P=P, Spre=c["kpre"].t.shape[1],
                Smax=SMAX_OWN, d_pos=c["d_pos"].data_ptr(), rot=64, sin=c["sin_t"].data_ptr(), cos=c["cos_t"].data_ptr(), ps=1)
    L = lib.load()

    def prefix(a):
        return L.mg_attn_decode_prefix_bf16(a["qkv"], a["kpre"], a["vpre"], a["part"], a["B"], a["H"], a["P"], a["Spre"], a["d_pos"],
                                            a["rot"], a["sin"], a["cos"], a["ps"], stream)

    def fused(a):
        return L.mg_attn_decode_fused_shared_bf16(a["qkv"], a["kown"], a["vown"], a["out"], a["B"], a["H"], a["Smax"], a["d_pos"],
                                                  a["rot"], a["sin"], a["cos"], a["ps"], a["P"], a["part"], stream)

    def gemv(a):
        return L.mg_decode_attn_gemv_shared_bf16(a["qkv"], a["kown"], a["vown"], a["out"], 0, a["B"], a["H"], a["Smax"], a["d_pos"],
                                                 a["rot"], a["sin"], a["cos"], C.byref(desc), a["ps"], a["P"], a["part"], stream)

    common = [("B", 17), ("B", 0), ("P", 0), ("P", -3), ("P", 4097), ("ps", 0), ("ps", 2), ("rot", 12), ("rot", 264), ("qkv", None),
              ("part", None), ("d_pos", None), ("sin", None), ("qkv", base["qkv"] + 2), ("part", base["part"] + 4)]
    cases = {
        "mg_attn_decode_prefix_bf16": (prefix, common + [("kpre", None), ("vpre", None), ("kpre", base["kpre"] + 2), ("Spre", P - 1)]),
        "mg_attn_decode_fused_shared_bf16": (fused, common + [("kown", None), ("vown", None), ("out", None), ("Smax", 4097), ("Smax", 0),
                                                              ("kown", base["kown"] + 2), ("out", base["out"] + 2)]),
        "mg_decode_attn_gemv_shared_bf16": (gemv, common + [("kown", None), ("vown", None), ("out", None), ("Smax", 4097), ("Smax", 0),
                                                            ("vown", base["vown"] + 2), ("out", base["out"] + 2)]),
    }
    snap = [t.view(torch.int16).clone() for t in (c["kown"].flat, c["vown"].flat, out.flat)]
    for name, (fn, bad) in cases.items():
        for key, value in bad:
            rc = fn({**base, key: value})
            assert rc != 0, (name, key, value)
            with pytest.raises(MagmaHipError, match=name):
                lib.check(rc, name)
    torch.cuda.synchronize()
    assert bool(c["part"].flat.isnan().all()) and bool(y.isnan().all())
    assert all(torch.equal(a, b.view(torch.int16)) for a, b in zip(snap, (c["kown"].flat, c["vown"].flat, out.flat)))
    for fn in (prefix, fused, gemv):            # the arguments themselves are good
        assert fn(base) == 0
    torch.cuda.synchronize()
    assert not bool(out.t.isnan().any()) and out.guards_intact()
