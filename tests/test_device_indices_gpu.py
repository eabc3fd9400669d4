"""The device-index contract (include/magma_hip.h "Device-resident indices"; the table: DESIGN.md), one parametrised case per row of
the table: a value a kernel reads from device memory and steers an address with -- a KV position, the step counter, a token id, a
parent, a source row, a trie node -- is planted two and one below its range, at its limit and one above, on the first and on the
last row of the batch, beside ordinary rows that carry the in-range edges 0 and limit - 1.  Asserted for every case:
  (a) both guard bands of every operand are intact;
  (b) bit for bit, every operand holds what it held before the launch plus what the contract permits the launch to write -- for a
      skipped row nothing, its output row included;
  (c) the ordinary rows carry exactly the bits of the same launch without the offending rows (where a value is one of several in a
      row -- a history token, an angle offset -- the launch with that value replaced by a harmless in-range one);
  (d) decode attention: the in-range edge rows also meet the fp64 per-element bound of test_kernels_gpu.assert_decode_attention.
device_indices.py says why no planted value can leave the test's own allocation, guarded or not."""
import pytest
import torch

import device_indices as di
from device_indices import BF16, Guarded, Operands, OUTSIDE, assert_decode_attention, outside, rnd, same_bits

pytestmark = pytest.mark.gpu

B, H, DH, D = 3, 2, 256, 512
SMAX, LAYERS, HC, T, ROT = 64, 2, 8, 5, 64
P_SHARED = 65                   # n_prefix of the shared-prefix launches: two chunks, the second one key long
VS = (64, 1056)
WHERE = ("first", "last")
I32, I64, F32 = torch.int32, torch.int64, torch.float32


def plant(which: str, where: str, limit: int, n: int = B):
    """n index values: the planted one on the first or the last row, the in-range edges 0 and limit - 1 on the others (in turn).
    -> (values, ordinary rows)."""
    row = 0 if where == "first" else n - 1
    ok = [r for r in range(n) if r != row]
    vals = [outside(which, limit)] * n
    for i, r in enumerate(ok):
        vals[r] = (0, limit - 1)[i % 2]
    return vals, ok


def i32(xs, dev):
    return torch.tensor(xs, dtype=I32, device=dev)


# ============================================================================================================ decode attention
def decode_operands(dev, pos, seed, rows=None, keys=None):
    """The operands of one fused decode launch for the rows ``rows`` (default: all) of the case (pos, seed): qkv [n, 3 D]; K / V
    caches that hold random keys below each row's position and the NaN pattern from it on (the append slot included; an offending
    row: the pattern everywhere); the output rows and the rotary tables of SMAX positions.  keys: other key counts per row."""
    rows = list(range(len(pos))) if rows is None else rows
    keys = [p if 0 <= p < SMAX else 0 for p in pos] if keys is None else keys
    n = len(rows)
    qkv = rnd(len(pos), 3 * D, dev=dev, seed=seed, scale=0.5).to(BF16)[rows].contiguous()
    k0 = rnd(len(pos), H, SMAX, DH, dev=dev, seed=seed + 1, scale=0.5).to(BF16)
    v0 = rnd(len(pos), H, SMAX, DH, dev=dev, seed=seed + 2).to(BF16)
    kc, vc = Guarded((n, H, SMAX, DH), BF16, dev), Guarded((n, H, SMAX, DH), BF16, dev)
    for i, r in enumerate(rows):
        m = keys[r]
        kc.t[i, :, :m], vc.t[i, :, :m] = k0[r, :, :m], v0[r, :, :m]
    sin_t, cos_t = di.tables(ROT, SMAX, dev)
    ops_ = Operands(kc=kc, vc=vc, out=Guarded((n, D), BF16, dev), sin=sin_t, cos=cos_t)
    return qkv, i32([pos[r] for r in rows], dev), ops_


def gemv_beside(dev):
    from magma_amd import ops
    x = rnd(B, 512, dev=dev, seed=84).to(BF16)
    lin = ops.PackedLinear(rnd(264, 512, dev=dev, seed=85, scale=0.05).to(BF16), bias=rnd(264, dev=dev, seed=86))
    return x, lin


def launch_decode(kind, qkv, d_pos, o, dev, pos_stride=1):
    """kind: "fused" (mg_attn_decode_fused_bf16) or "gemv" (mg_decode_attn_gemv_bf16) -> the co-launched GEMV's output or None."""
    from magma_amd import ops
    n = qkv.shape[0]
    args = (qkv, o["kc"].t, o["vc"].t, o["out"].t, n, H, d_pos, ROT, o["sin"].t, o["cos"].t)
    if kind == "fused":
        ops.attn_decode_fused(*args, pos_stride=pos_stride)
        return None
    x, lin = gemv_beside(dev)
    y = torch.empty(B, 264, dtype=F32, device=dev)
    ops.decode_attn_gemv(*args, (x, lin, y, {"out_dtype": F32}), pos_stride=pos_stride)
    return y


def rotated_q(qkv, d_pos, o, dev):
    """q of every row rotated at its position by the rotary launch (which the fused kernels equal bit for bit: test_kernels_gpu)."""
    from magma_amd import ops
    n = qkv.shape[0]
    q = torch.empty(n, H, 1, DH, dtype=BF16, device=dev)
    sink = [torch.empty(n, H, SMAX, DH, dtype=BF16, device=dev) for _ in range(2)]
    ops.rotary_split(qkv, n, 1, H, ROT, o["sin"].t, o["cos"].t, q, *sink, d_pos=d_pos, pos_stride=1)
    return q


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
@pytest.mark.parametrize("kind", ["fused", "gemv"])
def test_fused_decode_position(dev, kind, which, where):
    """mg_attn_decode_fused_bf16 / mg_decode_attn_gemv_bf16, d_pos[b] (range [0, Smax)): the offending row appends nothing, attends
    over nothing and leaves its output row alone; an unguarded append lands two or one position in front of the (b, 0) cache --
    the front guard or the neighbouring row's last positions -- or behind (b, H - 1)."""
    pos, ok = plant(which, where, SMAX)
    qkv, d_pos, o = decode_operands(dev, pos, seed=10)
    o.snapshot()
    y = launch_decode(kind, qkv, d_pos, o, dev)
    qkv_r, d_pos_r, r = decode_operands(dev, pos, seed=10, rows=ok)
    y_r = launch_decode(kind, qkv_r, d_pos_r, r, dev)
    want = {n: o.expected(n) for n in ("kc", "vc", "out")}
    for i, b in enumerate(ok):
        want["kc"][b], want["vc"][b], want["out"][b] = r["kc"].t[i], r["vc"].t[i], r["out"].t[i]
        assert not bool(r["out"].t[i].isnan().any()) and not bool(r["kc"].t[i, :, pos[b]].isnan().any())
    o.check(f"{kind}, d_pos {pos}", **want)
    if y is not None:
        assert same_bits(y, y_r)
    # (d) the in-range edge rows (contexts of 1 and of Smax keys) against fp64
    q = rotated_q(qkv_r, d_pos_r, r, dev)
    assert_decode_attention(q, r["kc"].t, r["vc"].t, [pos[b] + 1 for b in ok], f"{kind}, edge rows at {[pos[b] for b in ok]}", r["out"].t)


@pytest.mark.parametrize("which", OUTSIDE)
def test_fused_decode_one_position_for_the_batch(dev, which):
    """pos_stride 0: the one device position outside [0, Smax) skips every row -- last (b, h) and first alike."""
    p = outside(which, SMAX)
    qkv, _, o = decode_operands(dev, [p] * B, seed=11)
    o.snapshot()
    launch_decode("fused", qkv, i32([p], dev), o, dev, pos_stride=0)
    o.check(f"fused, one position {p}")


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
def test_plain_decode_position(dev, which, where):
    """mg_attn_decode_bf16 (q rotated, K / V appended by an earlier launch): the caches are only read; the offending row's output
    row stays as it is."""
    from magma_amd import ops
    pos, ok = plant(which, where, SMAX)

    def run(rows):
        qkv, d_pos, o = decode_operands(dev, pos, seed=12, rows=rows, keys=[p + 1 if 0 <= p < SMAX else 0 for p in pos])    # keys [0, pos]
        q = qkv[:, :D].reshape(len(rows), H, 1, DH).contiguous()
        o.snapshot()
        ops.attn_decode(q, o["kc"].t, o["vc"].t, o["out"].t, len(rows), H, d_pos, pos_stride=1)
        return q, o
    _, o = run(list(range(B)))
    q_r, r = run(ok)
    want = o.expected("out")
    for i, b in enumerate(ok):
        want[b] = r["out"].t[i]
    o.check(f"attn_decode, d_pos {pos}", out=want)
    assert_decode_attention(q_r, r["kc"].t, r["vc"].t, [pos[b] + 1 for b in ok], "attn_decode, edge rows", r["out"].t)


# ============================================================================================================ shared prefix
def shared_operands(dev, pos, seed, rows=None):
    """decode_operands for the shared-prefix launches: own caches of SMAX positions behind a prefix of P_SHARED, tables of
    P_SHARED + SMAX positions, the prefix itself and the partials guarded as well.  pos: absolute positions."""
    rows = list(range(len(pos))) if rows is None else rows
    own = [p - P_SHARED for p in pos]
    qkv, _, o = decode_operands(dev, own, seed, rows)
    qkv16 = torch.empty(16, 3 * D, dtype=BF16, device=dev)
    Guarded.fill_nan(qkv16)
    qkv16[:len(rows)] = qkv
    spre = 128
    kpre, vpre = Guarded((H, spre, DH), BF16, dev), Guarded((H, spre, DH), BF16, dev)
    kpre.t[:, :P_SHARED] = rnd(H, P_SHARED, DH, dev=dev, seed=seed + 3, scale=0.5).to(BF16)
    vpre.t[:, :P_SHARED] = rnd(H, P_SHARED, DH, dev=dev, seed=seed + 4).to(BF16)
    sin_t, cos_t = di.tables(ROT, P_SHARED + SMAX, dev)
    part = Guarded((len(rows), H, 2, 264), F32, dev)
    o = Operands(kc=o["kc"], vc=o["vc"], out=o["out"], sin=sin_t, cos=cos_t, kpre=kpre, vpre=vpre, part=part)
    return qkv16, i32([pos[r] for r in rows], dev), o


def launch_shared(kind, qkv16, d_pos, o, dev):
    from magma_amd import ops
    n = d_pos.numel()
    ops.attn_decode_prefix(qkv16, o["kpre"].t, o["vpre"].t, o["part"].t, n, H, P_SHARED, d_pos, ROT, o["sin"].t, o["cos"].t)
    args = (qkv16, o["kc"].t, o["vc"].t, o["out"].t, n, H, d_pos, ROT, o["sin"].t, o["cos"].t)
    kw = dict(pos_stride=1, shared=(P_SHARED, o["part"].t))
    if kind == "fused":
        ops.attn_decode_fused(*args, **kw)
        return None
    x, lin = gemv_beside(dev)
    y = torch.empty(B, 264, dtype=F32, device=dev)
    ops.decode_attn_gemv(*args, (x, lin, y, {"out_dtype": F32}), **kw)
    return y


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", ["limit", "limit+1"])
@pytest.mark.parametrize("kind", ["fused", "gemv"])
def test_shared_prefix_position_past_the_own_cache(dev, kind, which, where):
    """mg_attn_decode_prefix_bf16 + mg_attn_decode_fused_shared_bf16 / mg_decode_attn_gemv_shared_bf16, d_pos[b] (range
    [n_prefix, n_prefix + Smax); below n_prefix counts as n_prefix: test_shared_prefix_kernels_gpu): at or past n_prefix + Smax the
    row appends nothing -- it used to overwrite the row's last valid key -- and leaves its output alone.  The prefix launch has no
    Smax: it writes the row's partials (from an angle row one or two past the tables' n_prefix + Smax rows, i.e. the guard), which
    nothing reads; the other rows' partials are the reduced launch's."""
    own, ok = plant(which, where, SMAX)
    pos = [P_SHARED + p for p in own]
    qkv16, d_pos, o = shared_operands(dev, pos, seed=20)
    row = [b for b in range(B) if b not in ok][0]
    o["kc"].t[row], o["vc"].t[row] = rnd(H, SMAX, DH, dev=dev, seed=29).to(BF16), rnd(H, SMAX, DH, dev=dev, seed=30).to(BF16)   # a full row
    o.snapshot()
    y = launch_shared(kind, qkv16, d_pos, o, dev)
    qkv_r, d_pos_r, r = shared_operands(dev, pos, seed=20, rows=ok)
    y_r = launch_shared(kind, qkv_r, d_pos_r, r, dev)
    want = {n: o.expected(n) for n in ("kc", "vc", "out", "part")}
    want["part"][row] = o["part"].t[row]                          # the offending row's partials: written, never read
    for i, b in enumerate(ok):
        for n in ("kc", "vc", "out", "part"):
            want[n][b] = r[n].t[i]
        assert not bool(r["out"].t[i].isnan().any())
    o.check(f"shared {kind}, d_pos {pos}", **want)
    if y is not None:
        assert same_bits(y, y_r)


# ============================================================================================================ rotary + split
def chunk_positions(which, S=T):
    """First positions of a chunk of S rows whose first (low side) or last (high side) row lands two / one below 0, at Smax or one
    above; "0" and "top": the in-range edges."""
    return {"0": 0, "top": SMAX - S, "-2": -2, "-1": -1, "limit": SMAX - S + 1, "limit+1": SMAX - S + 2}[which]


def rotary_operands(dev, n, S, seed, rows_qkv):
    """qkv rows ``rows_qkv`` (of the case's B * T random rows), NaN-filled q_out [n, H, S, 256] and caches, guarded tables."""
    qkv = rnd(B * T, 3 * D, dev=dev, seed=seed, scale=0.5).to(BF16)[rows_qkv].contiguous()
    sin_t, cos_t = di.tables(ROT, SMAX, dev)
    return qkv, Operands(q=Guarded((n, H, S, DH), BF16, dev), kc=Guarded((n, H, SMAX, DH), BF16, dev),
                         vc=Guarded((n, H, SMAX, DH), BF16, dev), sin=sin_t, cos=cos_t)


def rotary_expected(dev, o, pos0, seed, launch):
    """What a chunk launch may write: per batch row b the rows s with pos0[b] + s inside [0, Smax), as ONE launch of B = 1 over
    exactly those rows (``launch(qkv, n, S, o, first position, s_lo)``) writes them."""
    want = {n: o.expected(n) for n in ("q", "kc", "vc")}
    for b, p in enumerate(pos0):
        s_ok = [s for s in range(T) if 0 <= p + s < SMAX]
        if not s_ok:
            continue
        qkv_r, r = rotary_operands(dev, 1, len(s_ok), seed, [b * T + s for s in s_ok])
        launch(qkv_r, 1, len(s_ok), r, p + s_ok[0], s_ok[0])
        want["q"][b][:, s_ok] = r["q"].t[0]
        lo, hi = p + s_ok[0], p + s_ok[-1] + 1
        want["kc"][b][:, lo:hi], want["vc"][b][:, lo:hi] = r["kc"].t[0][:, lo:hi], r["vc"].t[0][:, lo:hi]
        assert not bool(r["q"].t.isnan().any()) and not bool(r["kc"].t[0][:, lo:hi].isnan().any())
        assert di.is_pattern(r["kc"].t[0][:, :lo]) and di.is_pattern(r["kc"].t[0][:, hi:])
    return want


@pytest.mark.parametrize("which", ["0", "top", *OUTSIDE])
def test_rotary_split_device_scalar_position(dev, which):
    """mg_rotary_split_bf16 with a device scalar d_pos (pos_stride 0): a row s with *d_pos + s outside [0, Smax) is skipped; the
    unguarded kernel wrote it into the neighbouring (b, h) cache or the guard."""
    from magma_amd import ops
    p0 = chunk_positions(which)

    def launch(qkv, n, S, o, p, s_lo):
        ops.rotary_split(qkv, n, S, H, ROT, o["sin"].t, o["cos"].t, o["q"].t, o["kc"].t, o["vc"].t, d_pos=i32([p], dev))
    qkv, o = rotary_operands(dev, B, T, 40, list(range(B * T)))
    o.snapshot()
    launch(qkv, B, T, o, p0, 0)
    o.check(f"rotary_split, *d_pos = {p0}", **rotary_expected(dev, o, [p0] * B, 40, launch))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
def test_rotary_split_row_positions(dev, which, where):
    """mg_rotary_split_bf16 with one position per row (pos_stride 1)."""
    from magma_amd import ops
    row = 0 if where == "first" else B - 1
    pos0 = [chunk_positions(which) if b == row else chunk_positions(("0", "top")[(b + row) % 2]) for b in range(B)]

    def launch(qkv, n, S, o, p, s_lo):
        p = i32(p if isinstance(p, list) else [p], dev)
        ops.rotary_split(qkv, n, S, H, ROT, o["sin"].t, o["cos"].t, o["q"].t, o["kc"].t, o["vc"].t, d_pos=p, pos_stride=1)
    qkv, o = rotary_operands(dev, B, T, 41, list(range(B * T)))
    o.snapshot()
    launch(qkv, B, T, o, pos0, 0)
    o.check(f"rotary_split, d_pos {pos0}", **rotary_expected(dev, o, pos0, 41, launch))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
@pytest.mark.parametrize("through", ["slot", "angle"])
def test_rotary_split_at_slot_and_angle(dev, through, which, where):
    """mg_rotary_split_at_bf16: the slot d_pos[b] + s and the angle row d_pos[b] + off[b][s] are guarded apart.  "slot": the chunk
    position is planted (off = s).  "angle": one offset of the row puts the angle outside [0, Smax) while its slot is inside -- that
    row s alone is skipped, the others are those of the launch with the offset s (rows are independent)."""
    from magma_amd import ops
    row = 0 if where == "first" else B - 1
    off = torch.arange(T, dtype=I32, device=dev).repeat(B, 1)

    def launch(qkv, n, S, o, p, s_lo, off_=None):
        p = i32(p if isinstance(p, list) else [p], dev)
        off_ = (torch.arange(S, dtype=I32, device=dev) + 0).repeat(n, 1).contiguous() if off_ is None else off_
        ops.rotary_split_at(qkv, n, S, H, ROT, o["sin"].t, o["cos"].t, o["q"].t, o["kc"].t, o["vc"].t, p, off_)
    qkv, o = rotary_operands(dev, B, T, 42, list(range(B * T)))
    o.snapshot()
    if through == "slot":
        pos0 = [chunk_positions(which) if b == row else chunk_positions(("0", "top")[(b + row) % 2]) for b in range(B)]
        launch(qkv, B, T, o, pos0, 0, off)
        o.check(f"rotary_split_at, d_pos {pos0}", **rotary_expected(dev, o, pos0, 42, launch))
        return
    pos0, s_bad = [3, SMAX - T, 7], T - 1 if which.startswith("limit") else 0
    off[row, s_bad] = outside(which, SMAX) - pos0[row]
    launch(qkv, B, T, o, pos0, 0, off)
    want = rotary_expected(dev, o, pos0, 42, launch)
    slot = pos0[row] + s_bad
    for n in ("q", "kc", "vc"):
        before = o.expected(n)
        if n == "q":
            want[n][row][:, s_bad] = before[row][:, s_bad]
        else:
            want[n][row][:, slot] = before[row][:, slot]
    o.check(f"rotary_split_at, angle row {outside(which, SMAX)} for row {s_bad} of sequence {row}", **want)


# ============================================================================================================ chunk attention
def chunk_operands(dev, pos0, seed, rows=None, full=()):
    """q [n, H, T, 256] (rotated already), caches with random keys below p_b + T (rows in ``full``: everywhere) and the pattern
    beyond, the output rows [n T, D]."""
    rows = list(range(len(pos0))) if rows is None else rows
    n = len(rows)
    q = rnd(len(pos0), H, T, DH, dev=dev, seed=seed, scale=0.5).to(BF16)[rows].contiguous()
    k0 = rnd(len(pos0), H, SMAX, DH, dev=dev, seed=seed + 1, scale=0.5).to(BF16)
    v0 = rnd(len(pos0), H, SMAX, DH, dev=dev, seed=seed + 2).to(BF16)
    kc, vc = Guarded((n, H, SMAX, DH), BF16, dev), Guarded((n, H, SMAX, DH), BF16, dev)
    for i, r in enumerate(rows):
        m = SMAX if r in full else min(max(pos0[r], 0) + T, SMAX)
        kc.t[i, :, :m], vc.t[i, :, :m] = k0[r, :, :m], v0[r, :, :m]
    return q, i32([pos0[r] for r in rows], dev), Operands(kc=kc, vc=vc, out=Guarded((n * T, D), BF16, dev))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
@pytest.mark.parametrize("tree", [False, True])
def test_chunk_attention_position_is_clamped(dev, tree, which, where):
    """mg_attn_prefill_cached_bf16 / mg_attn_prefill_tree_bf16, d_pos[b]: CLAMPED into [0, Smax] before anything is derived from it (the
    header says so): a row below 0 is the row at 0, a row above Smax the row at Smax (a full cache: every key load lands on a slot
    <= Smax - 1).  The caches are only read; the ordinary rows are those of the launch without the offending row."""
    from magma_amd import ops
    row = 0 if where == "first" else B - 1
    planted = {"-2": -2, "-1": -1, "limit": SMAX + 1, "limit+1": SMAX + 2}[which]
    clamped = 0 if planted < 0 else SMAX
    edge = [1, SMAX - T] if tree else [0, SMAX - T]              # (the tree needs a cached key in front of it: p_min = 1)
    pos0 = [planted if b == row else edge[(b + row) % 2] for b in range(B)]
    as_clamped = [clamped if b == row else p for b, p in enumerate(pos0)]
    ok = [b for b in range(B) if b != row]
    sub = torch.full((B, T), T, dtype=I32, device=dev)

    def run(pos, rows=None):
        q, d_pos, o = chunk_operands(dev, as_clamped, 50, rows, full=(row,))
        rows = list(range(B)) if rows is None else rows
        d_pos = i32([pos[r] for r in rows], dev)
        o.snapshot()
        if tree:
            ops.attn_prefill_tree(q, o["kc"].t, o["vc"].t, o["out"].t, len(rows), H, T, d_pos, sub[rows].contiguous(), p_min=1, pos_stride=1)
        else:
            ops.attn_prefill_cached(q, o["kc"].t, o["vc"].t, o["out"].t, len(rows), H, T, d_pos, pos_stride=1)
        return o
    o, c, r = run(pos0), run(as_clamped), run(pos0, ok)
    want = c["out"].t.clone()
    for i, b in enumerate(ok):
        assert same_bits(c["out"].t[b * T:(b + 1) * T], r["out"].t[i * T:(i + 1) * T]), b
        assert not bool(r["out"].t[i * T:(i + 1) * T].isnan().any())
    o.check(f"chunk attention (tree {tree}), d_pos {pos0}", out=want)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
def test_tree_attention_subtree_end_is_a_mask_not_an_index(dev, which, where):
    """mg_attn_prefill_tree_bf16, sub[b][j] (range [j + 1, T]): only ever compared with a query index -- a value <= j hides key j from
    every query (as 0 does), a value > T shows it to every later query (as T does); no address depends on it."""
    from magma_amd import ops
    row = 0 if where == "first" else B - 1
    j = 0 if where == "first" else T - 1
    pos0 = [1, SMAX - T, 9]
    planted = outside(which, T)
    ok = [b for b in range(B) if b != row]

    def run(value, rows=None):
        q, d_pos, o = chunk_operands(dev, pos0, 51, rows)
        rows = list(range(B)) if rows is None else rows
        sub = torch.full((B, T), T, dtype=I32, device=dev)
        sub[row, j] = value
        o.snapshot()
        ops.attn_prefill_tree(q, o["kc"].t, o["vc"].t, o["out"].t, len(rows), H, T, d_pos, sub[rows].contiguous(), p_min=1, pos_stride=1)
        return o
    o, c, r = run(planted), run(0 if planted < 0 else T), run(T, ok)
    for i, b in enumerate(ok):
        assert same_bits(c["out"].t[b * T:(b + 1) * T], r["out"].t[i * T:(i + 1) * T]), b
    o.check(f"tree attention, sub[{row}][{j}] = {planted}", out=c["out"].t.clone())


# ============================================================================================================ KV row copies
def kv_caches(dev, R, seed):
    return [Guarded.of(rnd(LAYERS, R, H, SMAX, DH, dev=dev, seed=seed + i).to(BF16)) for i in range(2)]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
@pytest.mark.parametrize("through", ["parent", "d_pos"])
def test_kv_reorder(dev, through, which, where):
    """mg_kv_reorder_bf16: parent[b] outside [0, R) -- the row is skipped; d_pos CLAMPED into [0, Smax] (a count of positions: below 0
    nothing is copied, above Smax the whole row).  Against the indexed copy."""
    from magma_amd import ops
    R = 4
    row = 0 if where == "first" else R - 1
    parent, pos = [1, 2, 3, 0], [5, SMAX, 0, 17]                 # a cycle: every row is staged
    if through == "parent":
        parent[row] = outside(which, R)
    else:
        pos[row] = {"-2": -2, "-1": -1, "limit": SMAX + 1, "limit+1": SMAX + 2}[which]
    kc, vc = kv_caches(dev, R, 60)
    ks, vs = Guarded((LAYERS, R, H, SMAX, DH), BF16, dev), Guarded((LAYERS, R, H, SMAX, DH), BF16, dev)
    o = Operands(kc=kc, vc=vc, ks=ks, vs=vs).snapshot()
    ops.kv_reorder(kc.t, vc.t, ks.t, vs.t, i32(parent, dev), i32(pos, dev), pos_stride=1)
    cnt = [min(max(p, 0), SMAX) for p in pos]
    valid = [0 <= parent[b] < R for b in range(R)]
    staged = [valid[b] and parent[b] != b and any(c != b and parent[c] == b for c in range(R)) for b in range(R)]
    want = {n: o.expected(n) for n in ("kc", "vc", "ks", "vs")}
    for c_, s_ in (("kc", "ks"), ("vc", "vs")):
        src = o.expected(c_)
        for b in range(R):
            if staged[b]:
                want[s_][:, b, :, :cnt[b]] = src[:, b, :, :cnt[b]]
        for b in range(R):
            p = parent[b]
            if valid[b] and p != b:
                want[c_][:, b, :, :cnt[p]] = src[:, p, :, :cnt[p]]
    o.check(f"kv_reorder, parent {parent}, d_pos {pos}", **want)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
@pytest.mark.parametrize("through", ["src", "d_pos"])
def test_kv_broadcast(dev, through, which, where):
    """mg_kv_broadcast_bf16: src[b] outside the sample's own rows [b k, b k + k), or a position d_pos[r] + pos_delta outside
    [0, Smax): the row is skipped.  Against the indexed copy."""
    from magma_amd import ops
    k, R = 2, B * 2
    smp = 0 if where == "first" else B - 1
    src, pos = [1, 2, 5], [0, 0, SMAX - 1, SMAX - 1, 9, 9]
    if through == "src":
        src[smp] = smp * k + outside(which, k)
    else:
        r_bad = 0 if where == "first" else R - 1
        pos[r_bad if src[r_bad // k] != r_bad else r_bad - 1] = outside(which, SMAX)
    kc, vc = kv_caches(dev, R, 62)
    o = Operands(kc=kc, vc=vc).snapshot()
    ops.kv_broadcast(kc.t, vc.t, k, i32(src, dev), i32(pos, dev), pos_stride=1)
    want = {n: o.expected(n) for n in ("kc", "vc")}
    for n in want:
        before = o.expected(n)
        for r in range(R):
            s = src[r // k]
            if s != r and (r // k) * k <= s < (r // k) * k + k and 0 <= pos[r] < SMAX:
                want[n][:, r, :, pos[r]] = before[:, s, :, pos[r]]
    o.check(f"kv_broadcast, src {src}, d_pos {pos}", **want)


# ============================================================================================================ bookkeeping launches
def book(dev, step, n=B):
    """The guarded bookkeeping state of n rows at step ``step``: history [n, HC] of the pattern but for the columns before the step."""
    hist = Guarded((n, HC), I64, dev)
    for c in range(max(0, min(step, HC))):
        hist.t[:, c] = 20 + c
    return Operands(state=Guarded.of(i32([step, -1], dev)), d_pos=Guarded.of(i32([7 + b for b in range(n)], dev)),
                    token=Guarded.of(torch.tensor([30 + b for b in range(n)], dtype=I64, device=dev)), hist=hist,
                    finish=Guarded.of(i32([[-1, 0]] * n, dev)))


STEPS = ["0", "top", *OUTSIDE]


def step_of(which):
    return {"0": 0, "top": HC - 1}[which] if which in ("0", "top") else outside(which, HC)


@pytest.mark.parametrize("which", STEPS)
@pytest.mark.parametrize("kind", ["plain", "rows"])
def test_sample_finish_step(dev, kind, which):
    """mg_sample_finish / mg_sample_finish_rows, state[0] (history column, range [0, history_cols)): outside it no history column is
    written -- the plain launch used to write column -2 / -1 of row b, i.e. the neighbouring row's last columns or the guard --;
    the step counter and the positions advance as ever."""
    from magma_amd import ops
    step = step_of(which)
    o = book(dev, step).snapshot()
    if kind == "plain":
        ops.sample_finish(o["token"].t, 2, o["state"].t, o["d_pos"].t, 1, o["hist"].t, pos_stride=1)
    else:
        table = ops.stop_table([2, 3]).to(dev)
        ops.sample_finish_rows(o["token"].t, o["state"].t, table, 2, 0, 0, o["finish"].t, o["d_pos"].t, 1, o["hist"].t, pos_stride=1)
    want = {n: o.expected(n) for n in ("state", "d_pos", "hist")}
    want["state"][0] = step + 1
    want["d_pos"] += 1
    if 0 <= step < HC:
        want["hist"][:, step] = o.expected("token")
    o.check(f"sample_finish ({kind}), step {step}", **want)


@pytest.mark.parametrize("which", STEPS)
@pytest.mark.parametrize("through", ["step", "begin"])
def test_sample_finish_slots_ring(dev, through, which):
    """mg_sample_finish_slots: the history is a ring -- EVERY step maps to column step mod history_cols (in [0, history_cols) for a
    negative step too), and a window begin of any value gives a token count in [1, history_cols]: one column per row is written,
    whatever the two hold."""
    from magma_amd import ops
    v = step_of(which)
    step = v if through == "step" else 3
    o = book(dev, HC)                                            # a full ring
    o.bufs["slot"] = Guarded.of(i32([[v if through == "begin" else 0, 100]] * B, dev))
    o["state"].t[0] = step
    o.snapshot()
    table = ops.stop_table([2, 3]).to(dev)
    ops.sample_finish_slots(o["token"].t, o["state"].t, table, 2, 0, 0, o["finish"].t, o["slot"].t, o["hist"].t, o["d_pos"].t, 1)
    want = {n: o.expected(n) for n in ("state", "d_pos", "hist")}
    want["state"][0] = step + 1
    want["d_pos"] += 1
    want["hist"][:, step % HC] = o.expected("token")
    o.check(f"sample_finish_slots, step {step}, begin {o['slot'].t[0, 0].item()}", **want)


@pytest.mark.parametrize("which", ["-2", "-1", "0", "top"])
@pytest.mark.parametrize("entry", ["admit", "admit_at", "admit_shared"])
def test_slots_admit_step_and_first_token(dev, entry, which):
    """mg_slots_admit_bf16 / _at / _shared: every row, slot, length and offset is a HOST argument the entry point validates; from
    device memory come state[0] (the first token takes ring column (state[0] - 1) mod history_cols: any value lands in the ring) and
    the first tokens, which are stored and compared but never index anything -- ids two outside [0, V) included."""
    from magma_amd import ops
    step = {"-2": -1, "-1": 0, "0": 1, "top": HC}[which]        # state[0] - 1 = -2, -1, 0, HC - 1
    n_stage, s_stage = 2, 16
    pos0, dst0 = {"admit": (0, None), "admit_at": (3, None), "admit_shared": (3, 1)}[entry]
    ks = rnd(LAYERS, n_stage, H, s_stage, DH, dev=dev, seed=70).to(BF16)
    vs = rnd(LAYERS, n_stage, H, s_stage, DH, dev=dev, seed=71).to(BF16)
    kc, vc = kv_caches(dev, B, 72)
    o = book(dev, HC)
    o.bufs.update(kc=kc, vc=vc, slot=Guarded.of(i32([[0, 0]] * B, dev)))
    o["state"].t[0] = step
    o.snapshot()
    first = torch.tensor([-2, VS[0] + 1], dtype=I64, device=dev)
    src, dst, lens, limits = [1, 0], [B - 1, 0], [4, s_stage - pos0], [5, 5]
    table = ops.stop_table([2, 3]).to(dev)
    ops.slots_admit(ks, vs, kc.t, vc.t, src, dst, lens, first, limits, o["state"].t, o["d_pos"].t, o["token"].t, o["finish"].t,
                    o["slot"].t, o["hist"].t, table, 2, 0, pos0=pos0, dst0=dst0)
    want = {n: o.expected(n) for n in o.bufs}
    col, d0 = (step - 1) % HC, pos0 if dst0 is None else dst0
    for j in range(2):
        want["kc"][:, dst[j], :, d0:d0 + lens[j]] = ks[:, src[j], :, pos0:pos0 + lens[j]]
        want["vc"][:, dst[j], :, d0:d0 + lens[j]] = vs[:, src[j], :, pos0:pos0 + lens[j]]
        want["d_pos"][dst[j]], want["token"][dst[j]], want["hist"][dst[j], col] = pos0 + lens[j], first[j], first[j]
        want["slot"][dst[j]] = i32([col, limits[j]], dev)
        want["finish"][dst[j]] = i32([-1, 0], dev)
    want["state"][1] = -1
    o.check(f"{entry}, state[0] {step}", **want)


# ============================================================================================================ logits rows
def logits_rows(dev, V, seed, n=B):
    return Guarded.of(rnd(n, V, dev=dev, seed=seed))


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("which", OUTSIDE)
def test_logits_process_step_is_clamped(dev, which, V):
    """mg_logits_process_f32, state[0]: CLAMPED into [0, history_cols] -- the number of history columns the rules read (below 0: none,
    above history_cols: all of them)."""
    from magma_amd import ops
    step = {"-2": -2, "-1": -1, "limit": HC + 1, "limit+1": HC + 2}[which]

    def run(s):
        x = logits_rows(dev, V, 80)
        hist = Guarded.of(torch.tensor([[3, 5, 3, 5, 3, 5, 3, 5]] * B, dtype=I64, device=dev))
        o = Operands(x=x, hist=hist, state=Guarded.of(i32([s, -1], dev))).snapshot()
        ops.logits_process(x.t, o["state"].t, hist.t, repetition_penalty=1.5, no_repeat_ngram_size=2)
        return o
    o, c = run(step), run(0 if step < 0 else HC)
    o.check(f"logits_process, step {step}", x=c["x"].t.clone())
    assert (step < 0) == same_bits(c["x"].t, c.expected("x"))     # the rules did apply at the clamped step HC


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
@pytest.mark.parametrize("rule", ["penalty", "ngram"])
def test_logits_process_history_token(dev, rule, which, where, V):
    """mg_logits_process_f32, a history token outside [0, V): it is skipped by the repetition penalty (the offending row is the row
    whose bad tokens repeat a token it already holds) and as the banned token of an n-gram (nothing of the row changes); a stray
    x[V], x[V + 1] would be the next row's first logits (ld = V) or the guard."""
    from magma_amd import ops
    row = 0 if where == "first" else B - 1
    bad = outside(which, V)
    hist = [[5, 7, 5, 9, 11, 9, 13, 7] for _ in range(B)]
    same = [list(h) for h in hist]
    kw = dict(repetition_penalty=1.5) if rule == "penalty" else dict(no_repeat_ngram_size=2)
    if rule == "penalty":
        hist[row][1], hist[row][6], same[row][1], same[row][6] = bad, bad, 5, 5
        same[row][7], hist[row][7] = 5, 5
    else:                                                         # the last token 7 is followed by `bad` earlier on: its ban is skipped
        hist[row][2], same[row] = bad, None

    def run(h, keep=range(B)):
        x = Guarded.of(logits_rows(dev, V, 81).t[list(keep)].contiguous())
        o = Operands(x=x, hist=Guarded.of(torch.tensor(h, dtype=I64, device=dev)), state=Guarded.of(i32([HC, -1], dev))).snapshot()
        ops.logits_process(x.t, o["state"].t, o["hist"].t, **kw)
        return o
    o = run(hist)
    want = o.expected("x")
    if rule == "penalty":
        want = run(same)["x"].t.clone()
    else:
        ok = [b for b in range(B) if b != row]
        others = run([hist[b] for b in ok], ok)
        want[ok] = others["x"].t
        assert not same_bits(others["x"].t, others.expected("x"))
    o.check(f"logits_process ({rule}), token {bad} in row {row}", x=want)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
@pytest.mark.parametrize("through", ["path", "root"])
def test_constrained_logits_node_ids(dev, through, which, where):
    """mg_logits_process_constrained_f32: a cached path node or a root outside [0, n_nodes) -- the cache entry fails its own check and
    the walk starts over (the result is that of an empty cache), a row with such a root is off the trie (the eos ids alone)."""
    from magma_amd import ops, sampling
    V = VS[0]
    row = 0 if where == "first" else B - 1
    trie = sampling.TokenTrie([[5, 7, 9], [5, 8], [6]])
    table = trie.flat().to(dev)
    n_nodes = int(table[0])
    bad = outside(which, n_nodes)
    hist = torch.tensor([[5, 7] + [0] * (HC - 2)] * B, dtype=I64, device=dev)

    def run(path_value, root_value):
        x = logits_rows(dev, V, 82)
        path = Guarded.of(ops.trie_path(B, dev))
        roots = Guarded.of(torch.zeros(B, dtype=I32, device=dev))
        o = Operands(x=x, path=path, roots=roots, hist=Guarded.of(hist), state=Guarded.of(i32([2, -1], dev)),
                     table=Guarded.of(table))
        ops.logits_process_constrained(x.t, o["state"].t, hist, table, roots.t, path.t, eos=2)     # fills the path cache
        x.t.copy_(rnd(B, V, dev=dev, seed=82))
        if path_value is not None:
            path.t[row, 0 if where == "first" else 1] = path_value
        if root_value is not None:
            roots.t[row] = root_value
        o.snapshot()
        ops.logits_process_constrained(x.t, o["state"].t, o["hist"].t, o["table"].t, roots.t, path.t, eos=2)
        return o
    if through == "path":
        o, c = run(bad, None), run(None, None)
        o.check(f"constrained, path node {bad}", x=c["x"].t.clone(), path=c["path"].t.clone())
        assert int((c["x"].t[row] > float("-inf")).sum()) == 1   # after 5, 7 only 9 continues
    else:
        o, c = run(None, bad), run(None, None)
        want = c["x"].t.clone()
        want[row] = float("-inf")
        want[row, 2] = o.expected("x")[row, 2]
        o.check(f"constrained, root {bad}", x=want)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("which", STEPS)
def test_token_logprobs_step_column(dev, which, V):
    """mg_token_logprobs_f32, state[0] (the column of lp / top_id / top_lp, range [0, cols)): outside it nothing is written."""
    from magma_amd import ops
    step = step_of(which)

    def run(s):
        x = logits_rows(dev, V, 83)
        o = Operands(x=x, lp=Guarded((B, HC), F32, dev), top_id=Guarded((B, HC, 3), I32, dev), top_lp=Guarded((B, HC, 3), F32, dev),
                     token=Guarded.of(torch.tensor([0, V - 1, 7], dtype=I64, device=dev)), state=Guarded.of(i32([s, -1], dev))).snapshot()
        ops.token_logprobs(x.t, o["token"].t, o["lp"].t, o["top_id"].t, o["top_lp"].t, o["state"].t)
        return o
    o = run(step)
    if not 0 <= step < HC:
        o.check(f"token_logprobs, step {step}")
        return
    c = run(0)                                                    # the same rows into column 0
    want = {n: o.expected(n) for n in ("lp", "top_id", "top_lp")}
    for n in want:
        want[n][:, step] = c[n].t[:, 0]
    o.check(f"token_logprobs, step {step}", **want)
    assert not bool(o["lp"].t[:, step].isnan().any())


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
@pytest.mark.parametrize("entry", ["step", "rows: token", "rows: row"])
def test_token_logprobs_token_and_row(dev, entry, which, where, V):
    """mg_token_logprobs_f32 (token id) and mg_token_logprobs_rows_f32 (token id, logits row): a token outside [0, V) or a row outside
    [0, n_rows) reads nothing and gives -inf; the other entries are those of the launch without it."""
    from magma_amd import ops
    row = 0 if where == "first" else B - 1
    ok = [b for b in range(B) if b != row]
    tok = [0 if b % 2 else V - 1 for b in range(B)]
    rows_of = [0 if b % 2 else B - 1 for b in range(B)]
    if entry == "rows: row":
        rows_of[row] = outside(which, B)
    else:
        tok[row] = outside(which, V)

    def run(keep):
        x = logits_rows(dev, V, 84)
        if entry == "step":
            xs = Guarded.of(x.t[keep].contiguous())
            o = Operands(x=xs, lp=Guarded((len(keep), 1), F32, dev),
                         token=Guarded.of(torch.tensor([tok[b] for b in keep], dtype=I64, device=dev))).snapshot()
            ops.token_logprobs(xs.t, o["token"].t, o["lp"].t)
        else:
            o = Operands(x=x, lp=Guarded((len(keep),), F32, dev), token=Guarded.of(i32([tok[b] for b in keep], dev)),
                         row_of=Guarded.of(i32([rows_of[b] for b in keep], dev))).snapshot()
            ops.token_logprobs_rows(x.t, o["row_of"].t, o["token"].t, o["lp"].t)
        return o
    o, r = run(list(range(B))), run(ok)
    want = o.expected("lp")
    want[row] = float("-inf")
    for i, b in enumerate(ok):
        want[b] = r["lp"].t[i]
    assert bool(torch.isfinite(r["lp"].t).all())
    o.check(f"token_logprobs ({entry}), token {tok}, rows {rows_of}", lp=want)


# ============================================================================================================ row gathers
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
def test_embedding_id_is_clamped(dev, which, where):
    """mg_embedding_bf16, ids[b][t]: CLAMPED into [0, vocab) -- below 0 reads row 0, at or above vocab row vocab - 1."""
    from magma_amd import ops
    V, d = VS[0], 256
    ids = [[0, V - 1], [7, 8], [V - 1, 0]]
    b, t = (0, 0) if where == "first" else (B - 1, 1)
    ids[b][t] = outside(which, V)
    wte = Guarded.of(rnd(V, d, dev=dev, seed=90).to(BF16))
    o = Operands(wte=wte, out=Guarded((B, 2, d), BF16, dev)).snapshot()
    ops.embedding(torch.tensor(ids, dtype=I64, device=dev), wte.t, o["out"].t)
    want = wte.t[torch.tensor(ids, device=dev).clamp(0, V - 1)]
    o.check(f"embedding, ids {ids}", out=want)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
def test_cross_entropy_target(dev, which, where, V):
    """mg_ce_rows_f32, tgt[r]: outside [0, V) the row's loss is 0 and nothing of the row is read."""
    from magma_amd import lib
    row = 0 if where == "first" else B - 1
    ok = [b for b in range(B) if b != row]
    tgt = [0 if b % 2 else V - 1 for b in range(B)]
    tgt[row] = outside(which, V)

    def run(keep):
        x = logits_rows(dev, V, 91)
        xs = Guarded.of(x.t[keep].contiguous())
        if row in keep:
            Guarded.fill_nan(xs.t[keep.index(row)])               # nothing of the offending row is read
        o = Operands(x=xs, loss=Guarded((len(keep),), F32, dev)).snapshot()
        t = torch.tensor([tgt[b] for b in keep], dtype=I64, device=dev)
        lib.check(lib.load().mg_ce_rows_f32(xs.t.data_ptr(), V, t.data_ptr(), o["loss"].t.data_ptr(), len(keep), V,
                                            torch.cuda.current_stream().cuda_stream), "mg_ce_rows_f32")
        return o
    o, r = run(list(range(B))), run(ok)
    want = o.expected("loss")
    want[row] = 0.0
    for i, b in enumerate(ok):
        want[b] = r["loss"].t[i]
    assert bool(torch.isfinite(r["loss"].t).all())
    o.check(f"ce_rows, targets {tgt}", loss=want)


# ============================================================================================================ contrastive search
CS_K, CS_D, CS_T = 2, 256, 40


def contrast_operands(dev, lens, step=0):
    ctx = Guarded((B, CS_T, CS_D), BF16, dev)
    full = rnd(B, CS_T, CS_D, dev=dev, seed=95).to(BF16)
    for b, n in enumerate(lens):
        m = min(max(n, 0), CS_T)
        ctx.t[b, :m] = full[b, :m]
    hist = Guarded((B * CS_K, HC), I64, dev)
    return Operands(ctx=ctx, hidden=Guarded.of(rnd(B * CS_K, CS_D, dev=dev, seed=96).to(BF16)), ctx_len=Guarded.of(i32(lens, dev)),
                    part=Guarded((B, 2, CS_K), F32, dev), src=Guarded.of(i32([0] * B, dev)), hist=hist,
                    token=Guarded.of(torch.tensor([40 + r for r in range(B * CS_K)], dtype=I64, device=dev)),
                    state=Guarded.of(i32([step, -1], dev)), d_pos=Guarded.of(i32([9] * (B * CS_K), dev)),
                    cand_p=Guarded.of(torch.tensor([[0.2, 0.7], [0.6, 0.3], [0.1, 0.5]], dtype=F32, device=dev)))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
def test_contrastive_sim_context_length_is_clamped(dev, which, where):
    """mg_contrastive_sim_bf16, ctx_len[b]: CLAMPED into [0, Tmax] (below 0: no position, every chunk empty; above Tmax: the whole
    store)."""
    from magma_amd import ops
    row = 0 if where == "first" else B - 1
    planted = {"-2": -2, "-1": -1, "limit": CS_T + 1, "limit+1": CS_T + 2}[which]
    lens = [planted if b == row else (0, CS_T)[(b + row) % 2] for b in range(B)]
    as_clamped = [min(max(n, 0), CS_T) for n in lens]

    def run(ls):
        o = contrast_operands(dev, as_clamped)
        o["ctx_len"].t.copy_(i32(ls, dev))
        o.snapshot()
        ops.contrastive_sim(o["hidden"].t, o["ctx"].t, o["ctx_len"].t, CS_K, o["part"].t, CS_T)
        return o
    o, c = run(lens), run(as_clamped)
    o.check(f"contrastive_sim, ctx_len {lens}", part=c["part"].t.clone())
    assert not bool(c["part"].t.isnan().any())


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
@pytest.mark.parametrize("through", ["ctx_len", "step"])
def test_contrastive_finish(dev, through, which, where):
    """mg_contrastive_finish: ctx_len[b] outside [0, Tmax) -- the selected hidden row is not appended and the length stays; state[0]
    outside [0, history_cols) -- no history column is written.  Selection, src, positions and the step counter as ever."""
    from magma_amd import ops
    row = 0 if where == "first" else B - 1
    lens = [3, 0, CS_T - 1]
    step = 0
    if through == "ctx_len":
        lens[row] = outside(which, CS_T)
    else:
        step = outside(which, HC)
    o = contrast_operands(dev, lens, step)
    o["part"].t.fill_(-1.0e30)                                    # no context position: the score is (1 - alpha) p
    o.snapshot()
    ops.contrastive_finish(o["part"].t, o["cand_p"].t, 0.6, o["hidden"].t, o["ctx"].t, o["ctx_len"].t, o["src"].t, o["token"].t, 2,
                           o["state"].t, CS_T - 1, o["d_pos"].t, 1, o["hist"].t, pos_stride=1)
    want = {n: o.expected(n) for n in ("ctx", "ctx_len", "src", "hist", "state", "d_pos")}
    sel = [1, 0, 1]
    for b in range(B):
        r = b * CS_K + sel[b]
        want["src"][b] = r
        if 0 <= lens[b] < CS_T:
            want["ctx"][b, lens[b]] = o.expected("hidden")[r]
            want["ctx_len"][b] = lens[b] + 1
        if 0 <= step < HC:
            want["hist"][b * CS_K:(b + 1) * CS_K, step] = o.expected("token")[r]
    want["state"][0] = step + 1
    want["d_pos"] += 1
    o.check(f"contrastive_finish, ctx_len {lens}, step {step}", **want)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("which", OUTSIDE)
def test_contrastive_topk_source_row_is_clamped(dev, which, where):
    """mg_contrastive_topk_f32, src[b]: outside the sample's rows [b k, b k + k) it counts as the sample's first row b k."""
    from magma_amd import ops
    V = VS[0]
    smp = 0 if where == "first" else B - 1
    src = [1, 2, 5]
    as_clamped = list(src)
    src[smp], as_clamped[smp] = smp * CS_K + outside(which, CS_K), smp * CS_K

    def run(s):
        o = Operands(x=logits_rows(dev, V, 97, n=B * CS_K), token=Guarded((B * CS_K,), I64, dev), cand_p=Guarded((B, CS_K), F32, dev),
                     src=Guarded.of(i32(s, dev))).snapshot()
        ops.contrastive_topk(o["x"].t, o["src"].t, CS_K, o["token"].t, o["cand_p"].t)
        return o
    o, c = run(src), run(as_clamped)
    o.check(f"contrastive_topk, src {src}", token=c["token"].t.clone(), cand_p=c["cand_p"].t.clone())


# ============================================================================================================ beam bookkeeping
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("which", OUTSIDE)
@pytest.mark.parametrize("through", ["token", "step"])
def test_beam_finish(dev, through, which, grouped):
    """mg_beam_finish / mg_beam_finish_groups.  Candidate tokens (from the top-k launch) are VALUES -- ranked with, stored, compared
    with eos -- and the parents are formed inside the launch from list positions, always inside the sample's rows: a token outside
    [0, V) on the first and the last candidate changes nothing but the stored token itself.  state[0] below 0 gathers no history
    column and writes none; at or above the histories' ld it gathers ld columns and writes none."""
    from magma_amd import ops
    V, k, G = VS[1], 4, 2                                        # (1056 ids: every candidate token is a different one)
    R, ld = B * k, HC
    K2 = k + k // G if grouped else 2 * k
    step = outside(which, ld) if through == "step" else 3
    g = torch.Generator().manual_seed(5)
    score = -torch.rand(R, K2, generator=g).sort(1).values.contiguous()          # descending per row, all different
    tok = (torch.randperm(V - 3, generator=g)[:R * K2] + 3).to(I32).view(R, K2).contiguous()

    def run(tokens, s):
        f32z = lambda *sh: Guarded.of(torch.zeros(*sh, dtype=F32, device=dev))       # noqa: E731
        bufs = dict(run=f32z(R), fin_score=Guarded.of(torch.full((R,), -1.0e9, dtype=F32, device=dev)),
                    fin_flag=Guarded.of(torch.zeros(R, dtype=I32, device=dev)), fin_len=Guarded.of(torch.zeros(R, dtype=I32, device=dev)),
                    unsat=Guarded.of(torch.ones(B * (G if grouped else 1), dtype=I32, device=dev)),
                    parent=Guarded((R,), I32, dev), token=Guarded((R,), I64, dev))
        for name in ("fin_tok", "fin_stage", "hist", "hist_stage"):
            bufs[name] = Guarded((R, ld), I64, dev)
        cols = max(0, min(s, ld))
        bufs["hist"].t[:, :cols] = torch.arange(R * cols, device=dev).view(R, cols) + 100
        bufs["fin_tok"].t[:, :cols] = 2
        o = Operands(cand_score=Guarded.of(score.to(dev)), cand_tok=Guarded.of(tokens.to(dev)), state=Guarded.of(i32([s, -1], dev)),
                     d_pos=Guarded.of(i32([11] * R, dev)), **bufs).snapshot()
        plain = {n: b.t for n, b in bufs.items()}
        if grouped:
            ops.beam_finish_groups(o["cand_score"].t, o["cand_tok"].t, B, k, G, 0.5, V, 2, 1.0, False, 50, o["state"].t, plain, o["d_pos"].t, 1)
        else:
            ops.beam_finish(o["cand_score"].t, o["cand_tok"].t, B, k, V, 2, 1.0, False, 50, o["state"].t, plain, o["d_pos"].t, 1)
        return o
    if through == "token":
        bad = tok.clone()
        bad[0, 0], bad[R - 1, 0] = outside(which, V), outside(which, V)
        o, c = run(bad, step), run(tok, step)
        want = {n: c[n].t.clone() for n in o.bufs if n not in ("cand_tok",)}
        for n in ("token", "hist", "fin_tok"):                   # the stored token itself differs, nothing else
            differs = o[n].t != c[n].t
            assert bool(((o[n].t == outside(which, V)) | ~differs).all()), n
            want[n] = torch.where(differs, o[n].t, c[n].t)
        assert bool(((o["parent"].t >= 0) & (o["parent"].t < R)).all())
        o.check(f"beam_finish (groups {grouped}), candidate token {outside(which, V)}", **want)
        return
    o = run(tok, step)
    want = {n: o.expected(n) for n in o.bufs}
    torch.cuda.synchronize()
    for n in ("run", "fin_score", "fin_flag", "fin_len", "unsat", "parent", "token", "hist_stage", "fin_stage"):
        want[n] = o[n].t.clone()                                  # values: whatever the merge decides
    cols = max(0, min(step, ld))
    assert bool(((o["parent"].t >= 0) & (o["parent"].t < R)).all())
    want["hist"][:, :cols] = o["hist_stage"].t[o["parent"].t.long(), :cols] if cols else want["hist"][:, :0]
    want["fin_tok"] = o["fin_tok"].t.clone()
    want["fin_tok"][:, cols:] = o.expected("fin_tok")[:, cols:]
    want["state"] = o["state"].t.clone()
    want["state"][0] = step + 1
    want["d_pos"] += 1
    assert di.is_pattern(o["hist_stage"].t[:, cols:]) and di.is_pattern(o["fin_stage"].t[:, cols:])
    o.check(f"beam_finish (groups {grouped}), step {step}", **want)
