"""The two kernels of speculative greedy decoding (DESIGN.md "Speculative decoding"), each against the statement it must equal
exactly:
  mg_attn_decode_chunk_bf16  against T successive mg_attn_decode_fused_bf16 launches on a copy of the cache, row t fed at position
                             pos_b + t: the bits of out and of both caches, every operand between 4 KiB guard bands;
  mg_spec_finish             against sampling.speculate_update on random states, the degenerate device values included.
No tolerance anywhere: the feature is exact because these equalities are."""
import ctypes as C

import pytest
import torch

import device_indices as di
from device_indices import BF16, Guarded, Operands, rnd

pytestmark = pytest.mark.gpu

H, DH, D, SMAX, ROT = 2, 256, 512, 320, 64
I32, I64 = torch.int32, torch.int64
# contexts that cross the 16-key wave step, the 64-key sweep and the 256-thread stride, inside a chunk too
POSITIONS = (0, 1, 14, 15, 16, 17, 62, 63, 64, 65, 255, 256, 300)


def i32(xs, dev):
    """int32 values; a sum past 2^31 - 1 wraps as the device's does."""
    return torch.tensor([(int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31 for x in xs], dtype=I32, device=dev)


# ============================================================================================================ chunk attention
def chunk_operands(dev, pos, T, seed, ld_out=D):
    """qkv [B*T, 3 D]; caches with random keys below every row's position and the NaN pattern from it on; NaN-filled out rows of
    stride ld_out; the rotary tables of SMAX positions.  Twice: for the chunk launch and for the T single-query launches."""
    B = len(pos)
    qkv = rnd(B * T, 3 * D, dev=dev, seed=seed, scale=0.5).to(BF16)
    k0 = rnd(B, H, SMAX, DH, dev=dev, seed=seed + 1, scale=0.5).to(BF16)
    v0 = rnd(B, H, SMAX, DH, dev=dev, seed=seed + 2).to(BF16)

    def one():
        kc, vc = Guarded((B, H, SMAX, DH), BF16, dev), Guarded((B, H, SMAX, DH), BF16, dev)
        for b, p in enumerate(pos):
            m = min(max(p, 0), SMAX)
            kc.t[b, :, :m], vc.t[b, :, :m] = k0[b, :, :m], v0[b, :, :m]
        sin_t, cos_t = di.tables(ROT, SMAX, dev)
        return Operands(kc=kc, vc=vc, out=Guarded((B * T, ld_out), BF16, dev), sin=sin_t, cos=cos_t)
    return qkv, one(), one()


def successive(qkv, pos, T, rot, ref, dev):
    """The statement: launch t feeds row t of every sequence at position pos_b + t (one position per row)."""
    from magma_amd import ops
    B = len(pos)
    for t in range(T):
        out_t = Guarded((B, D), BF16, dev)
        ops.attn_decode_fused(qkv[t::T].contiguous(), ref["kc"].t, ref["vc"].t, out_t.t, B, H, i32([p + t for p in pos], dev), rot,
                              ref["sin"].t, ref["cos"].t, pos_stride=1)
        torch.cuda.synchronize()
        assert out_t.guards_intact()
        ref["out"].t[t::T, :D] = out_t.t


def chunk_case(dev, pos, T, rot, seed, pos_stride=1, ld_out=D):
    from magma_amd import ops
    B = len(pos)
    qkv, got, ref = chunk_operands(dev, pos, T, seed, ld_out)
    got.snapshot()
    d_pos = i32(pos if pos_stride else pos[:1], dev)
    args = (qkv, got["kc"].t, got["vc"].t, got["out"].t[:, :D], B, T, H, d_pos, rot, got["sin"].t, got["cos"].t)
    ops.attn_decode_chunk(*args, pos_stride=pos_stride)
    successive(qkv, pos, T, rot, ref, dev)
    what = f"chunk B={B} T={T} rot={rot} pos={pos}"
    got.check(what, kc=ref["kc"].t, vc=ref["vc"].t, out=ref["out"].t)            # guards, and every operand to the bit
    for b, p in enumerate(pos):
        for t in range(T):
            row = got["out"].t[b * T + t, :D]
            if 0 <= p + t < SMAX:
                assert not bool(row.isnan().any()), f"{what}: live row ({b}, {t}) holds a NaN"
                assert not bool(got["kc"].t[b, :, p + t].isnan().any()) and not bool(got["vc"].t[b, :, p + t].isnan().any())
            else:
                assert di.is_pattern(row), f"{what}: dead row ({b}, {t}) was written"
    if ld_out > D:
        assert di.is_pattern(got["out"].t[:, D:]), f"{what}: columns behind H*256 of the out rows were written"


def groups(B):
    """Every value of POSITIONS in some launch, mixed within the batch."""
    vals = list(POSITIONS)
    while len(vals) % B:
        vals.append(POSITIONS[len(vals) % len(POSITIONS)])
    return [vals[i::len(vals) // B][:B] for i in range(len(vals) // B)]


@pytest.mark.parametrize("rot", [0, ROT])
@pytest.mark.parametrize("B,T", [(1, 2), (1, 3), (1, 4), (1, 5), (1, 8), (3, 2), (3, 3), (3, 4), (3, 5), (2, 8)])
def test_chunk_attention_has_the_bits_of_successive_launches(dev, B, T, rot):
    seen = set()
    for i, pos in enumerate(groups(B)):
        chunk_case(dev, pos, T, rot, seed=20 + i)
        seen.update(pos)
    assert seen == set(POSITIONS)


@pytest.mark.parametrize("T", [2, 5, 8])
def test_chunk_rows_outside_the_cache_are_dead(dev, T):
    """Per row: pos_b + t at or past Smax, or below 0, appends nothing, attends over nothing and leaves its out row alone, while the
    chunk's other rows are the successive launches' (which skip by the same rule).  d_pos = -1: row 0 is dead, row t > 0 sits at
    t - 1; d_pos = Smax - 2: rows 0 and 1 live; d_pos = Smax + 5 and -T: the whole chunk is dead."""
    for pos in ([SMAX - 2], [-1], [SMAX + 5], [-T], [SMAX - 1], [2 ** 31 - 1], [-2 ** 31]):
        chunk_case(dev, pos, T, ROT, seed=40)
    chunk_case(dev, [SMAX - 2, 17], T, ROT, seed=41)
    chunk_case(dev, [64, -1], T, ROT, seed=42)


@pytest.mark.parametrize("T", [3, 8])
def test_chunk_one_shared_position_and_wide_out_rows(dev, T):
    chunk_case(dev, [63, 63], T, ROT, seed=50, pos_stride=0)
    chunk_case(dev, [300], T, 0, seed=51, pos_stride=0)
    chunk_case(dev, [15, 256], T, ROT, seed=52, ld_out=D + 264)


def test_chunk_refusals_come_before_any_launch(dev):
    from magma_amd import lib as L
    fn = L.load().mg_attn_decode_chunk_bf16
    qkv, o, _ = chunk_operands(dev, [5, 6], 4, seed=60)
    o.snapshot()
    d_pos = i32([5, 6], dev)
    big = torch.empty(16, dtype=BF16, device=dev)           # a cache pointer for the Smax no launch may reach

    def call(qkv_p=qkv.data_ptr(), kc=o["kc"].t.data_ptr(), out=o["out"].t.data_ptr(), ld_out=D, B=2, T=4, Smax=SMAX,
             pos=d_pos.data_ptr(), rot=ROT, sin=o["sin"].t.data_ptr(), ps=1):
        return fn(qkv_p, kc, o["vc"].t.data_ptr(), out, ld_out, B, T, H, Smax, pos, rot, sin, o["cos"].t.data_ptr(), ps, None)

    def message():
        return L.load().mg_last_error().decode()

    for kw, word in ((dict(T=1), "2 <= T <= 8"), (dict(T=9), "2 <= T <= 8"), (dict(B=5), "at most 16 rows"), (dict(B=0), "Smax"),
                     (dict(Smax=0), "Smax"), (dict(Smax=4097), "Smax"), (dict(ps=2), "pos_stride"), (dict(rot=12), "rot_dim"),
                     (dict(rot=264), "rot_dim"), (dict(pos=None), "null pointer"), (dict(qkv_p=None), "null pointer"),
                     (dict(sin=None), "null pointer"), (dict(qkv_p=qkv.data_ptr() + 2), "16-byte aligned"),
                     (dict(out=o["out"].t.data_ptr() + 2), "16-byte aligned"), (dict(ld_out=D - 8), "ld_out"),
                     (dict(ld_out=D + 4), "ld_out"), (dict(T=8, kc=big.data_ptr(), Smax=4096), "LDS")):
        rc = call(**kw)
        assert rc != 0 and word in message(), (kw, rc, message())
    o.check("refusals")                                     # nothing was launched: every operand is as it was
    assert call() == 0                                      # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert not bool(o["out"].t.isnan().any())


# ------------------------------------------------------------------------------------------------------------- the co-launch
def gemv_beside(dev, rows, K, seed=84):
    from magma_amd import ops
    x = rnd(rows, K, dev=dev, seed=seed).to(BF16)
    lin = ops.PackedLinear(rnd(264, K, dev=dev, seed=seed + 1, scale=0.05).to(BF16), bias=rnd(264, dev=dev, seed=seed + 2))
    return x, lin


def plain_gemv(dev, x, lin):
    """The GEMV output of the plain co-launch over the same M rows (its attention runs on operands of its own)."""
    from magma_amd import ops
    M = x.shape[0]
    qkv, o, _ = chunk_operands(dev, [3] * M, 1, seed=90)
    y = Guarded((M, 264), torch.float32, dev)
    ops.decode_attn_gemv(qkv, o["kc"].t, o["vc"].t, o["out"].t, M, H, i32([3] * M, dev), ROT, o["sin"].t, o["cos"].t,
                         (x, lin, y.t, {"out_dtype": torch.float32}), pos_stride=1)
    torch.cuda.synchronize()
    assert y.guards_intact() and not bool(y.t.isnan().any())
    return y.t.clone()


def co_launch_case(dev, pos, T, rot, seed, K, pos_stride=1, ld_out=D):
    """chunk_case through mg_decode_attn_gemv_chunk_bf16: the attention part as there, the GEMV part against the plain co-launch."""
    from magma_amd import ops
    B = len(pos)
    qkv, got, ref = chunk_operands(dev, pos, T, seed, ld_out)
    x, lin = gemv_beside(dev, B * T, K)
    y = Guarded((B * T, 264), torch.float32, dev)
    got.snapshot()
    ops.decode_attn_gemv(qkv, got["kc"].t, got["vc"].t, got["out"].t[:, :D], B, H, i32(pos if pos_stride else pos[:1], dev), rot,
                         got["sin"].t, got["cos"].t, (x, lin, y.t, {"out_dtype": torch.float32}), pos_stride=pos_stride, chunk=T)
    successive(qkv, pos, T, rot, ref, dev)
    what = f"co-launch B={B} T={T} rot={rot} pos={pos} K={K}"
    got.check(what, kc=ref["kc"].t, vc=ref["vc"].t, out=ref["out"].t)
    assert y.guards_intact(), what
    assert torch.equal(y.t, plain_gemv(dev, x, lin)), f"{what}: the GEMV differs from the plain co-launch's over the same M"


@pytest.mark.parametrize("K", [128, 512, 2048])                # the GEMV instantiations of 1, 4 and 16 k-step quads
@pytest.mark.parametrize("B,T", [(1, 2), (3, 3), (3, 5), (1, 8), (2, 8)])
def test_co_launch_attention_and_gemv(dev, B, T, K):
    for i, pos in enumerate(groups(B)[:: 2 if B == 1 else 1]):
        co_launch_case(dev, pos, T, ROT if i % 2 else 0, seed=120 + i, K=K)


def test_co_launch_dead_rows_shared_position_and_wide_out_rows(dev):
    for T in (2, 8):
        for pos in ([SMAX - 2], [-1], [SMAX + 5], [64, -1]):
            co_launch_case(dev, pos, T, ROT, seed=140, K=512)
        co_launch_case(dev, [63, 63], T, ROT, seed=141, K=512, pos_stride=0)
        co_launch_case(dev, [15, 256], T, ROT, seed=142, K=512, ld_out=D + 264)


def test_co_launch_refusals_come_before_the_launch(dev):
    """Every refusal of either part returns before the one launch: the caches, the out rows and the GEMV output keep their fill --
    also when the attention part is fine and only the GEMV's descriptor (or its K, the ladder's last refusal) is not."""
    from magma_amd import lib as L, ops
    fn = L.load().mg_decode_attn_gemv_chunk_bf16
    qkv, o, _ = chunk_operands(dev, [5, 6], 4, seed=160)
    x, lin = gemv_beside(dev, 8, 512)
    y = Guarded((8, 264), torch.float32, dev)
    o.bufs["y"] = y
    o.snapshot()
    d_pos = i32([5, 6], dev)
    big = torch.empty(16, dtype=BF16, device=dev)

    def desc(**fields):
        d = ops.skinny_desc(x, lin, y.t, out_dtype=torch.float32)[0]
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    def call(d=None, kc=o["kc"].t.data_ptr(), out=o["out"].t.data_ptr(), ld_out=D, B=2, T=4, Smax=SMAX, rot=ROT, ps=1, gemv=True):
        d = d if d is not None else desc()
        return fn(qkv.data_ptr(), kc, o["vc"].t.data_ptr(), out, ld_out, B, T, H, Smax, d_pos.data_ptr(), rot, o["sin"].t.data_ptr(),
                  o["cos"].t.data_ptr(), C.byref(d) if gemv else None, ps, None)

    for kw, word in ((dict(T=1), "2 <= T <= 8"), (dict(T=0), "2 <= T <= 8"), (dict(T=9), "2 <= T <= 8"), (dict(B=5), "at most 16 rows"),
                     (dict(Smax=4097), "Smax"), (dict(ps=2), "pos_stride"), (dict(rot=12), "rot_dim"),
                     (dict(out=o["out"].t.data_ptr() + 2), "16-byte aligned"), (dict(ld_out=D + 4), "ld_"),
                     (dict(T=8, kc=big.data_ptr(), Smax=4096), "LDS"), (dict(gemv=False), ""), (dict(d=desc(split_n=8)), "split_n"),
                     (dict(d=desc(Kp=96)), "Kp"), (dict(d=desc(Kp=64)), "multiple of 128"), (dict(d=desc(W=None)), ""), (dict(d=desc(M=17)), "")):
        rc = call(**kw)
        assert rc != 0 and word in L.load().mg_last_error().decode(), (kw, rc, L.load().mg_last_error().decode())
    o.check("co-launch refusals")                           # nothing was launched: no K / V appended, no out row, no GEMV row
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(o["out"].t.isnan().any()) and not bool(y.t.isnan().any())


def test_chunk_lds_fits_gptj_window(dev):
    """T = 8 at Smax = 2048 (GPT-J's window) fits a workgroup's LDS: the launch runs above 64 KB of dynamic LDS and equals the
    successive launches at the window's last positions."""
    from magma_amd import ops
    S, T = 2048, 8
    pos = [S - T]
    qkv = rnd(T, 3 * D, dev=dev, seed=70, scale=0.5).to(BF16)
    k0 = rnd(1, H, S, DH, dev=dev, seed=71, scale=0.5).to(BF16)
    v0 = rnd(1, H, S, DH, dev=dev, seed=72).to(BF16)
    sin_t, cos_t = di.tables(ROT, S, dev)
    kc, vc, out = Guarded.of(k0), Guarded.of(v0), Guarded((T, D), BF16, dev)
    kr, vr, outr = Guarded.of(k0), Guarded.of(v0), Guarded((T, D), BF16, dev)
    ops.attn_decode_chunk(qkv, kc.t, vc.t, out.t, 1, T, H, i32(pos, dev), ROT, sin_t.t, cos_t.t, pos_stride=1)
    for t in range(T):
        ops.attn_decode_fused(qkv[t:t + 1].contiguous(), kr.t, vr.t, outr.t[t:t + 1], 1, H, i32([pos[0] + t], dev), ROT, sin_t.t,
                              cos_t.t, pos_stride=1)
    torch.cuda.synchronize()
    for a, b in ((kc, kr), (vc, vr), (out, outr)):
        assert a.guards_intact() and b.guards_intact() and di.same_bits(a.t, b.t)
    assert not bool(out.t.isnan().any())


# ================================================================================================================ spec_finish
VOCAB, EOS_IDS = 6, (5,)
POISON64 = 0x7FC17FC17FC17FC1


def spec_state(B, T, cols, lcols, seed, arm=False, eos_ids=EOS_IDS):
    """A random state of the loop on the host: tokens below the vocabulary (matches are common), counts near 0 and near the
    history's width, lookup lengths of 0, 1 and lcols, drafts that agree with the step's argmaxes for a random prefix, some rows
    finished.  Bytes no correct launch reads hold the NaN pattern."""
    g = torch.Generator().manual_seed(seed)

    def r(lo, hi, *shape):
        return torch.randint(lo, hi, shape, generator=g)
    live = VOCAB - len(eos_ids) if seed % 3 else VOCAB          # mostly no eos among the random tokens
    st = dict(ids=r(0, live, B, T).to(I64), n_draft=r(0, T, B).to(I32), token=r(0, VOCAB, B if arm else B * T).to(I64),
              history=torch.full((B, cols), POISON64, dtype=I64), count=torch.zeros(B, dtype=I32),
              finish=torch.tensor([[-1, 0]] * B, dtype=I32), pos=r(0, 100, B).to(I32), stats=r(0, 9, B, 3).to(I32),
              lookup=torch.full((B, lcols), 0x7FC17FC1, dtype=I32), lookup_len=torch.zeros(B, dtype=I32),
              state=torch.tensor([int(r(0, 50, 1)), -1], dtype=I32))
    for b in range(B):
        c = 0 if arm else int((1, 2, cols - 1, cols - 2, cols // 2)[int(r(0, 5, 1))])
        st["count"][b] = c
        st["history"][b, :c] = r(0, live, c)
        n = (0, 1, lcols)[int(r(0, 3, 1))] if lcols else 0
        st["lookup_len"][b] = n
        st["lookup"][b, :n] = r(0, live, n).to(I32)
        if arm:
            st["n_draft"][b] = 0
        else:                                               # the drafts agree with the argmaxes for a random prefix
            agree = int(r(0, T, 1))
            st["ids"][b, 1:1 + agree] = st["token"][b * T:b * T + agree]
        if not arm and int(r(0, 4, 1)) == 0:
            st["finish"][b] = torch.tensor([c, 0x100], dtype=I32)
    return st


def run_both(dev, st, T, num_tokens, max_ngram, limit, arm=False, eos_ids=EOS_IDS):
    """The host statement on a copy, the launch on guarded device copies; everything compared exactly."""
    from magma_amd import ops
    from magma_amd.sampling import speculate_update
    want = {k: v.clone() for k, v in st.items()}
    speculate_update(want["ids"], want["n_draft"], want["token"], want["history"], want["count"], want["finish"], want["pos"],
                     want["stats"], want["lookup"], want["lookup_len"], want["state"], num_tokens=num_tokens, max_ngram=max_ngram,
                     eos_ids=eos_ids, limit=limit, arm=arm, vocab=VOCAB)
    got = Operands(**{k: Guarded.of(v.to(dev)) for k, v in st.items()})
    table = ops.stop_table(eos_ids).to(dev)
    ops.spec_finish(got["ids"].t, got["n_draft"].t, got["token"].t, got["history"].t, got["count"].t, got["finish"].t, table,
                    len(eos_ids), limit, got["lookup"].t, got["lookup_len"].t, got["stats"].t, got["state"].t, num_tokens,
                    max_ngram, VOCAB, got["pos"].t, arm=arm)
    torch.cuda.synchronize()
    for k in st:
        assert got[k].guards_intact(), f"a guard band of `{k}` was written"
        assert torch.equal(got[k].t.cpu(), want[k]), (k, got[k].t.cpu(), want[k], st[k])
    return want


@pytest.mark.parametrize("lcols", [0, 1, 50])
@pytest.mark.parametrize("B,T", [(1, 2), (1, 4), (1, 8), (3, 2), (3, 4), (2, 8), (8, 2)])
def test_spec_finish_equals_the_host_statement(dev, B, T, lcols):
    cols = 24
    for seed in range(12):
        eos = EOS_IDS if seed % 2 else (5, 0, 3)
        st = spec_state(B, T, cols, lcols, seed * 7 + B + T, eos_ids=eos)
        run_both(dev, st, T, num_tokens=1 + seed % (T - 1), max_ngram=1 + seed % 4, limit=(cols, cols - 1, 12)[seed % 3], eos_ids=eos)
    for seed in range(4):
        st = spec_state(B, T, cols, lcols, 100 + seed, arm=True)
        run_both(dev, st, T, num_tokens=T - 1, max_ngram=2, limit=cols, arm=True)


def test_spec_finish_named_cases(dev):
    """The cases of the CPU test on the device: full, partial and zero acceptance, an eos inside the accepted run, the limit
    cutting the run, a frozen row, the arming call -- with the outcome stated here, not only compared."""
    T, cols = 4, 16

    def state(ids, nd, token, hist, finish=(-1, 0), lookup=()):
        h = torch.full((1, cols), POISON64, dtype=I64)
        h[0, :len(hist)] = torch.tensor(hist, dtype=I64)
        lk = torch.full((1, 8), 0x7FC17FC1, dtype=I32)
        lk[0, :len(lookup)] = torch.tensor(lookup, dtype=I32)
        return dict(ids=torch.tensor([ids], dtype=I64), n_draft=torch.tensor([nd], dtype=I32), token=torch.tensor(token, dtype=I64),
                    history=h, count=torch.tensor([len(hist)], dtype=I32), finish=torch.tensor([list(finish)], dtype=I32),
                    pos=torch.tensor([40], dtype=I32), stats=torch.zeros(1, 3, dtype=I32), lookup=lk,
                    lookup_len=torch.tensor([len(lookup)], dtype=I32), state=torch.tensor([3, -1], dtype=I32))
    kw = dict(T=T, num_tokens=3, max_ngram=2, limit=cols)
    w = run_both(dev, state([1, 2, 3, 4], 3, [2, 3, 4, 1], [0, 1]), **kw)                      # full: 4 tokens
    assert w["count"].tolist() == [6] and w["pos"].tolist() == [44] and w["stats"].tolist() == [[1, 3, 3]]
    assert w["history"][0, :6].tolist() == [0, 1, 2, 3, 4, 1]
    w = run_both(dev, state([1, 2, 3, 4], 3, [2, 0, 4, 1], [0, 1]), **kw)                      # partial: draft 2 wrong -> 2 tokens
    assert w["count"].tolist() == [4] and w["history"][0, :4].tolist() == [0, 1, 2, 0] and w["stats"].tolist() == [[1, 3, 1]]
    w = run_both(dev, state([1, 2, 3, 4], 3, [4, 3, 4, 1], [0, 1]), **kw)                      # zero: the model's own token only
    assert w["count"].tolist() == [3] and w["pos"].tolist() == [41] and w["stats"].tolist() == [[1, 3, 0]]
    w = run_both(dev, state([1, 2, 5, 4], 3, [2, 5, 4, 1], [0, 1]), **kw)                      # eos inside the accepted run: kept, cut
    assert w["count"].tolist() == [4] and w["finish"].tolist() == [[4, 0x100]] and w["n_draft"].tolist() == [0]
    assert w["ids"].tolist() == [[5] * T] and w["state"].tolist() == [4, 3]
    w = run_both(dev, state([1, 2, 3, 4], 3, [2, 3, 4, 1], [0, 1]), T=T, num_tokens=3, max_ngram=2, limit=4)   # the limit cuts
    assert w["count"].tolist() == [4] and w["finish"].tolist() == [[4, 0x300]]
    w = run_both(dev, state([1, 2, 3, 4], 3, [2, 3, 4, 1], [0, 1], finish=(2, 0x100)), **kw)  # frozen
    assert w["count"].tolist() == [2] and w["pos"].tolist() == [40] and w["stats"].tolist() == [[0, 0, 0]]
    w = run_both(dev, state([0, 0, 0, 0], 0, [2], [], lookup=[1, 2, 3, 4, 1]), arm=True, **kw)  # arming: token 0, first drafts
    assert w["count"].tolist() == [1] and w["pos"].tolist() == [40] and w["ids"].tolist() == [[2, 3, 4, 1]]
    assert w["n_draft"].tolist() == [3]


@pytest.mark.parametrize("what", ["n_draft", "count_negative", "count_past", "lookup_len", "lookup_len_negative"])
def test_spec_finish_degenerate_device_values(dev, what):
    """Values no correct loop leaves in device memory: n_draft > T - 1, a negative count, a count past the history, a lookup_len
    beyond the buffer.  Nothing outside the operands is written (run_both looks at every guard band), the other rows are the host
    statement's, and so is the offending row under the stated clamps."""
    B, T, cols, lcols = 3, 4, 24, 50
    for row in (0, B - 1):
        st = spec_state(B, T, cols, lcols, 200 + row)
        st["finish"][row] = torch.tensor([-1, 0], dtype=I32)
        if what == "n_draft":
            st["n_draft"][row] = T + 2
        elif what == "count_negative":
            st["count"][row] = -2
        elif what == "count_past":
            st["count"][row] = cols + 2
        elif what == "lookup_len":
            st["lookup_len"][row] = lcols + 2
        else:
            st["lookup_len"][row] = -2
        run_both(dev, st, T, num_tokens=T - 1, max_ngram=3, limit=cols)


def test_spec_finish_refusals_come_before_the_launch(dev):
    from magma_amd import lib as L, ops
    fn = L.load().mg_spec_finish
    B, T, cols, lcols = 2, 4, 24, 50
    st = spec_state(B, T, cols, lcols, 300)
    g = Operands(**{k: Guarded.of(v.to(dev)) for k, v in st.items()})
    table = ops.stop_table(EOS_IDS).to(dev)
    g.snapshot()
    p = {k: g[k].t.data_ptr() for k in st}

    def call(ids=p["ids"], B=B, T=T, n_draft=p["n_draft"], token=p["token"], ts=T, history=p["history"], ld_h=cols, cols=cols,
             count=p["count"], finish=p["finish"], table=table.data_ptr(), n_eos=1, limit=cols, d_pos=p["pos"], lookup=p["lookup"],
             ld_l=lcols, lcols=lcols, lookup_len=p["lookup_len"], stats=p["stats"], state=p["state"], num_tokens=T - 1, max_ngram=2,
             vocab=VOCAB):
        return fn(ids, B, T, n_draft, token, ts, history, ld_h, cols, count, finish, table, n_eos, limit, d_pos, lookup, ld_l, lcols,
                  lookup_len, stats, state, num_tokens, max_ngram, vocab, None)

    cases = [(dict(T=1), "T"), (dict(T=9), "T"), (dict(B=0), "T"), (dict(B=5), "B * T"), (dict(ts=2), "token_stride"),
             (dict(ts=0), "token_stride"), (dict(cols=0), "history"), (dict(ld_h=cols - 1), "history"), (dict(lcols=-1), "lookup"),
             (dict(ld_l=lcols - 1), "lookup"), (dict(n_eos=0), "n_eos"), (dict(n_eos=9), "n_eos"), (dict(num_tokens=0), "num_tokens"),
             (dict(num_tokens=T), "num_tokens"), (dict(max_ngram=0), "max_ngram"), (dict(max_ngram=17), "max_ngram"),
             (dict(limit=-1), "limit"), (dict(vocab=0), "vocab"), (dict(count=p["count"] + 2), "4-byte"),
             (dict(state=p["state"] + 1), "4-byte"), (dict(ids=p["ids"] + 4), "8-byte"), (dict(history=p["history"] + 4), "8-byte"),
             (dict(token=p["token"] + 4), "8-byte")]
    cases += [(dict(**{k: None}), "null pointer") for k in ("ids", "n_draft", "token", "history", "count", "finish", "table",
                                                              "lookup", "lookup_len", "stats", "state")]
    for kw, word in cases:
        rc = call(**kw)
        assert rc != 0 and word in L.load().mg_last_error().decode(), (kw, rc, L.load().mg_last_error().decode())
    g.check("spec_finish refusals")                         # nothing was launched
    assert call() == 0 and call(d_pos=None, ts=1) == 0      # the step's call and the arming call's form run
    torch.cuda.synchronize()
    assert all(g[k].guards_intact() for k in st)
