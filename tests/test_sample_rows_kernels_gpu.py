"""Per-request sampling, the kernel (csrc/sampling.hip, the TableRows instances of sample_kernel; mg_sample_rows_f32; DESIGN.md
"Per-request sampling"): ops.sample_rows against the FLAT kernels launched on every row alone.

The claim is a construction, not a tolerance: row r of a per-row launch runs the flat kernel's body with the scalars of its record
and draws at the Philox counter (j, 0) under its own seed -- the key and counter of row 0 of a one-row flat call at state[0] = j.
So every comparison here is bit equality (torch.equal on tokens, on the int32 view of the filtered rows), and nothing is measured."""
import struct

import pytest
import torch

from device_indices import Guarded, Operands

pytestmark = pytest.mark.gpu

SAMPLERS = (False, True)            # warp: the reference's filters / transformers' sampler


def _logits(R, V, seed=0):
    """Rows with ties: even rows are quantised to 1/8 (ties at every top-k threshold and, where the maximum repeats, at the
    maximum), every fourth row has its maximum planted twice, the rest are plain N(0, 3^2)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=g) * 3.0
    x[::2] = (x[::2] * 8).round() / 8
    for r in range(0, R, 4):
        m = float(x[r].max()) + 0.5
        x[r, (7 * r + 3) % V], x[r, (11 * r + V // 2) % V] = m, m
    return x


# (temperature, top_k, top_p, min_p); min_p is read by transformers' sampler only
GRID = ((0.7, 0, 0.9, 0.0), (0.0, 0, 0.9, 0.0), (1.3, 40, 0.0, 0.1), (0.7, 1, 1.0, 0.0), (1.0, 60000, 0.9, 0.1),
        (0.7, 40, 0.9, 0.0), (1.3, 5, 0.3, 0.0), (1.0, 0, 0.0, 0.0), (0.7, 0, 1.0, 0.1))


def _records(R, warp, grid=GRID):
    recs = []
    for r in range(R):
        t, k, p, m = grid[r % len(grid)]
        recs.append((t, k, p, m if warp else 0.0, 1000003 * r + 17))
    return recs


def _table(recs, dev):
    from magma_amd import ops
    return ops.sample_rows_table(*zip(*recs)).to(dev)


def _flat(x_row, rec, counter, warp):
    """(token, filtered row) of the flat kernel on this row ALONE with the record's scalars and seed at state[0] = counter; a
    greedy record: ops.argmax and the row with its first maximum alone."""
    from magma_amd import ops
    t, k, p, m, seed = rec
    dev = x_row.device
    x1 = x_row[None]
    if t == 0.0:
        tok = ops.argmax(x1)
        f = torch.full_like(x1, float("-inf"))
        f[0, tok[0]] = x1[0, tok[0]]
        return tok, f
    sd = torch.tensor([seed], dtype=torch.int64, device=dev)
    st = torch.tensor([counter, -1], dtype=torch.int32, device=dev)
    f = torch.empty_like(x1)
    if warp:
        tok = ops.sample_warp(x1, t, k, p, m, sd, st, filtered=f)
    else:
        tok = ops.sample(x1, t, k, p, sd, st, filtered=f)
    return tok, f


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("warp", SAMPLERS)
@pytest.mark.parametrize("V", [50258, 1000])
@pytest.mark.parametrize("R", [1, 5, 16, 300])
def test_row_equals_flat_call(dev, R, V, warp):
    from magma_amd import ops
    x = _logits(R, V, seed=R + V).to(dev)
    recs = _records(R, warp)
    counter = 3 + R % 5
    state = torch.tensor([counter, -1], dtype=torch.int32, device=dev)
    f = torch.full_like(x, float("nan"))
    tok = ops.sample_rows(x, _table(recs, dev), state, warp, filtered=f)
    only = ops.sample_rows(x, _table(recs, dev), state, warp)                     # without the filtered output: the same tokens
    assert torch.equal(tok, only)
    want_tok, want_f = zip(*[_flat(x[r], recs[r], counter, warp) for r in range(R)])
    want_tok, want_f = torch.cat(want_tok), torch.cat(want_f)
    bad = (tok != want_tok).nonzero().flatten().tolist()
    assert not bad, (bad, [recs[r] for r in bad])
    assert _same_bits(f, want_f), (f != want_f).any(1).nonzero().flatten().tolist()
    assert state.tolist() == [counter, -1]                                        # read, never written


@pytest.mark.parametrize("warp", SAMPLERS)
def test_mixed_tables_in_one_launch(dev, warp):
    """Greedy beside sampled rows, top_k 0 / 1 / 40 / >= V, top_p 0 / 0.9 / 1 and min_p 0 / 0.1 in ONE launch; rows 12.. share
    logits and settings: equal seeds give equal tokens, different seeds are free to differ (over 8 seeds of a flat distribution of
    1000 tokens they do)."""
    from magma_amd import ops
    V = 1000
    mp = 0.1 if warp else 0.0
    rows = [(0.0, 0, 0.9, 0.0), (0.7, 0, 0.9, 0.0), (1.3, 0, 0.9, 0.0), (0.7, 1, 0.9, 0.0), (0.7, 40, 0.9, 0.0), (0.7, V, 0.9, 0.0),
            (0.7, V + 7, 0.9, 0.0), (0.7, 0, 0.0, 0.0), (0.7, 0, 1.0, 0.0), (0.7, 0, 0.0, mp), (1.3, 40, 0.9, mp), (0.0, 40, 0.0, 0.0)]
    recs = [(*s, 100 + i) for i, s in enumerate(rows)]
    shared = (1.3, 0, 0.0, 0.0)
    recs += [(*shared, 7000 + i) for i in range(8)] + [(*shared, 7000), (*shared, 7003)]
    R = len(recs)
    x = _logits(R, V, seed=5)
    x[12:] = torch.randn(V, generator=torch.Generator().manual_seed(6)) * 0.5
    x = x.to(dev)
    state = torch.tensor([2, -1], dtype=torch.int32, device=dev)
    f = torch.empty_like(x)
    tok = ops.sample_rows(x, _table(recs, dev), state, warp, filtered=f)
    for r in range(R):
        wt, wf = _flat(x[r], recs[r], 2, warp)
        assert int(tok[r]) == int(wt[0]) and _same_bits(f[r:r + 1], wf), (r, recs[r])
    t = tok.tolist()
    assert t[20] == t[12] and t[21] == t[15]                 # equal seeds, equal rows: equal tokens
    assert len(set(t[12:20])) >= 2                           # different seeds: not one token for all
    assert t[3] == int(x[3].argmax())                        # top_k = 1 keeps the maximum alone


@pytest.mark.parametrize("V", [50258, 1000, 65])
def test_greedy_rows_equal_argmax(dev, V):
    from magma_amd import ops
    R = 7
    x = _logits(R, V, seed=V).to(dev)
    recs = [(0.0, 40, 0.9, 0.0, 5 + r) for r in range(R)]
    state = torch.tensor([9, -1], dtype=torch.int32, device=dev)
    for warp in SAMPLERS:
        assert torch.equal(ops.sample_rows(x, _table(recs, dev), state, warp), ops.argmax(x))
    # (row 0 has its maximum twice: the first one wins)
    assert int(ops.argmax(x)[0]) == int((x[0] == x[0].max()).nonzero()[0])


@pytest.mark.parametrize("warp", SAMPLERS)
def test_slot_form_counters_and_idle_rows(dev, warp):
    """A slot session's tables: the counter of row r is the number of tokens its occupant has so far -- the length of
    sampling.slot_tokens' window, which is slot_update's count n minus 1 at this step (n includes the token the step selects).  The
    solo call draws its j-th token at state[0] = j, and slot_tokens returns exactly j tokens then.  Over a ring of 8 columns and
    steps 1 .. 20 (more than two wraps).  Finished / idle rows and a row whose begin lies outside the ring hold NaN logits: their
    token keeps its sentinel, and every other output is what it is with finite logits there."""
    from magma_amd import ops
    from magma_amd.sampling import slot_tokens
    R, V, cols = 6, 1000, 8
    x = (torch.randn(R, V, generator=torch.Generator().manual_seed(3)) * 0.5).to(dev)
    recs = [(0.9, 0, 0.0, 0.0, 31 + r) for r in range(R)]
    recs[4] = (0.0, 0, 0.0, 0.0, 0)
    table = _table(recs, dev)
    ring = torch.zeros(R, cols, dtype=torch.int64)
    seen = set()
    for step in range(1, 21):
        begins = [(step - 1 - (r * 3 + step // 5) % cols) % cols for r in range(R)]       # windows of 1 .. cols tokens
        begins[5] = (-1, cols, cols + 1)[step % 3]                                         # outside the ring: skipped
        idle = [r == step % 5 for r in range(R)]
        slot = torch.tensor([[b, 99] for b in begins], dtype=torch.int32, device=dev)
        fin = torch.tensor([[step - 1, 0x300] if i else [-1, 0] for i in idle], dtype=torch.int32, device=dev)
        state = torch.tensor([step, -1], dtype=torch.int32, device=dev)
        skipped = [r for r in range(R) if idle[r] or r == 5]
        xn = x.clone()
        xn[skipped] = float("nan")
        out = {}
        for name, lg in (("finite", x), ("nan", xn)):
            tok = torch.full((R,), -7, dtype=torch.int64, device=dev)
            f = torch.full_like(x, 123.0)
            ops.sample_rows(lg, table, state, warp, out=tok, filtered=f, slot=slot, finish=fin, history_cols=cols)
            out[name] = (tok, f)
        assert torch.equal(out["finite"][0], out["nan"][0]) and _same_bits(out["finite"][1], out["nan"][1])
        tok, f = out["nan"]
        for r in range(R):
            if r in skipped:
                assert int(tok[r]) == -7 and bool((f[r] == 123.0).all()), (step, r)
                continue
            n = len(slot_tokens(ring[r], begins[r], step, cols))
            seen.add(n)
            wt, wf = _flat(x[r], recs[r], n, warp)
            assert int(tok[r]) == int(wt[0]) and _same_bits(f[r:r + 1], wf), (step, r, n)
    assert seen == set(range(1, cols + 1))


def test_refusals_leave_outputs_alone(dev):
    from magma_amd import lib, ops
    R, V = 4, 1000
    x = _logits(R, V).to(dev)
    table = _table(_records(R, True), dev)
    spare = torch.zeros(R * ops.SAMPLE_ROW_BYTES + 16, dtype=torch.uint8, device=dev)
    state = torch.tensor([0, -1], dtype=torch.int32, device=dev)
    slot = torch.zeros(R, 2, dtype=torch.int32, device=dev)
    fin = torch.full((R, 2), -1, dtype=torch.int32, device=dev)
    tok = torch.full((R,), -7, dtype=torch.int64, device=dev)
    f = torch.full_like(x, float("nan"))
    fn = lib.load().mg_sample_rows_f32

    def call(**kw):
        a = dict(logits=x.data_ptr(), ld=V, R=R, V=V, warp=1, params=table.data_ptr(), state=state.data_ptr(), slot=None,
                 finish=None, cols=0, token=tok.data_ptr(), filtered=f.data_ptr(), ldf=V)
        a.update(kw)
        return fn(a["logits"], a["ld"], a["R"], a["V"], a["warp"], a["params"], a["state"], a["slot"], a["finish"], a["cols"],
                  a["token"], a["filtered"], a["ldf"], None)

    bad = [dict(R=0), dict(R=-1), dict(V=0), dict(V=-3), dict(logits=None), dict(params=None), dict(state=None),
           dict(token=None, filtered=None), dict(ld=V - 1), dict(ldf=V - 1), dict(warp=2), dict(warp=-1),
           dict(finish=fin.data_ptr()),                                     # finish without slot
           dict(slot=slot.data_ptr()),                                      # slot without finish
           dict(slot=slot.data_ptr(), finish=fin.data_ptr(), cols=0),       # a ring of no columns
           dict(params=spare.data_ptr() + 8), dict(params=spare.data_ptr() + 4),   # the table: 16-byte aligned
           dict(logits=x.data_ptr() + 2), dict(state=state.data_ptr() + 1), dict(token=tok.data_ptr() + 4),
           dict(filtered=f.data_ptr() + 1), dict(slot=slot.data_ptr() + 2, finish=fin.data_ptr(), cols=8),
           dict(slot=slot.data_ptr(), finish=fin.data_ptr() + 2, cols=8)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert "mg_sample_rows_f32" in lib.load().mg_last_error().decode()
    torch.cuda.synchronize()
    assert bool((tok == -7).all()) and bool(torch.isnan(f).all())
    assert call() == 0 and call(slot=slot.data_ptr(), finish=fin.data_ptr(), cols=8) == 0       # the plain calls pass
    torch.cuda.synchronize()
    assert bool((tok >= 0).all()) and not bool(torch.isnan(f).any())
    with pytest.raises(AssertionError):
        ops.sample_rows(x, table[:-1], state)                              # ops: one record per row


@pytest.mark.parametrize("warp", SAMPLERS)
def test_degenerate_table_values(dev, warp):
    """The table is device memory no entry point can look at: a NaN, negative, zero or infinite temperature selects greedily, a
    negative top_k is off, a NaN / out-of-range top_p or log_min_p is off -- and every operand sits between 4 KiB guard bands of a
    NaN pattern that keep their fill."""
    from magma_amd import ops
    V = 1000
    nan, inf = float("nan"), float("inf")
    greedy = [(nan, 40, 0.9, 0.0), (-1.0, 40, 0.9, 0.0), (inf, 0, 0.9, 0.0), (-inf, 5, 0.5, 0.0), (-0.0, 0, 0.0, 0.0)]
    same_as = [((0.7, -1, 0.9, 0.0), (0.7, 0, 0.9, 0.0)), ((0.7, -2 ** 31, 0.0, 0.0), (0.7, 0, 0.0, 0.0)),
               ((0.7, 40, nan, 0.0), (0.7, 40, 0.0, 0.0)), ((0.7, 40, -3.0, 0.0), (0.7, 40, 0.0, 0.0)),
               ((0.7, 40, 7.0, 0.0), (0.7, 40, 0.0, 0.0))]
    recs = [(*s, 50 + i) for i, s in enumerate(greedy + [a for a, _ in same_as])]
    want = [(0.0, 0, 0.0, 0.0, 0)] * len(greedy) + [(*b, 50 + len(greedy) + i) for i, (_, b) in enumerate(same_as)]
    R = len(recs)
    table = _table(recs, dev)
    if warp:            # a NaN log(min_p) is off too (sample_rows_table never writes one: planted into the last record)
        table[R - 1, 8:16] = torch.tensor(list(struct.pack("<d", nan)), dtype=torch.uint8, device=dev)
    ops_ = Operands(logits=Guarded.of(_logits(R, V, seed=8).to(dev)), params=Guarded.of(table),
                    state=Guarded.of(torch.tensor([4, -1], dtype=torch.int32, device=dev)),
                    token=Guarded((R,), torch.int64, dev), filtered=Guarded((R, V), torch.float32, dev)).snapshot()
    x = ops_["logits"].t
    ops.sample_rows(x, ops_["params"].t, ops_["state"].t, warp, out=ops_["token"].t, filtered=ops_["filtered"].t)
    tok_w, f_w = zip(*[_flat(x[r], want[r], 4, warp) for r in range(R)])
    ops_.check("mg_sample_rows_f32, degenerate records", token=torch.cat(tok_w), filtered=torch.cat(f_w))
