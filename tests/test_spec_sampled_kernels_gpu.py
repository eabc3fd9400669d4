"""The two launches of speculative decoding for sampled rows and stop sequences, on bare kernels (DESIGN.md "Speculative
decoding"): mg_sample_chunk_f32 against the one-row mg_sample_rows_f32 call it is defined by -- token and filtered row, exactly --,
its skipped rows (NaN logits unread, outputs untouched), its degenerate device values and its refusals; mg_spec_finish_seq against
the host statement speculate_update(stop_seqs=...) on the cases of test_speculative_sampled_cpu.py, and against mg_spec_finish at
n_seq = 0.  Every comparison is an equality."""
import math

import pytest
import torch

from device_indices import Guarded, Operands
from test_spec_kernels_gpu import spec_state
from test_speculative_sampled_cpu import CASES, NAMED, host_update, run_case, token_by_token

pytestmark = pytest.mark.gpu

I32, I64, F32 = torch.int32, torch.int64, torch.float32
COLS = 40                                   # history_cols of the chunk tests
SENTINEL_TOKEN, SENTINEL_F = -99, 7.25
SHAPES = [(1, 2), (2, 8), (4, 4), (3, 5)]
# (temperature, top_k, top_p, min_p): top-k alone, top-p alone, a greedy record, min-p (read by transformers' sampler only: a
# wide nucleus beside it, so that the reference's filters drop something under this record too)
RECORDS = [(0.8, 40, 1.0, 0.0), (1.2, 0, 0.9, 0.0), (0.0, 0, 0.9, 0.0), (0.9, 0, 0.97, 0.05)]


def records(B, first, warp):
    rows = [RECORDS[(first + b) % 4] for b in range(B)]
    return [(t, k, p, m if warp else 0.0, 1000 + 17 * b) for b, (t, k, p, m) in enumerate(rows)]


def table_of(rows, dev):
    from magma_amd import ops
    return ops.sample_rows_table(*zip(*rows)).to(dev)


def logits_of(R, V, dev, seed):
    """fp32 [R, V] inside rows of ld = V + 13 floats (ld > V); a few exact ties at the top of every row."""
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(R, V + 13, generator=g) * 3.0
    for r in range(R):
        i = torch.randint(0, V, (3,), generator=g)
        wide[r, i] = wide[r, :V].max() + 0.5
    wide[:, V:] = float("nan")              # nothing behind a row's V logits is a logit
    return wide.to(dev)[:, :V]


def first_max(row):
    return int((row == row.max()).nonzero()[0])


def one_row_reference(logits, table, B, T, count, warp, live):
    """What the definition says: every live fed row alone through mg_sample_rows_f32 with its sequence's record at state[0] =
    count[b] + t.  {row: (token, filtered row)}."""
    from magma_amd import ops
    V, dev, want = logits.shape[1], logits.device, {}
    for r in live:
        b, t = divmod(r, T)
        state = torch.tensor([int(count[b]) + t, -1], dtype=I32, device=dev)
        filt = torch.full((1, V), SENTINEL_F, dtype=F32, device=dev)
        tok = ops.sample_rows(logits[r:r + 1], table[b:b + 1], state, warp, filtered=filt)
        want[r] = (int(tok[0]), filt[0].clone())
    return want


def run_chunk(logits, table, B, T, count, n_draft, finish, warp):
    """The launch on guarded, sentinel-filled outputs: (token [B * T], filtered [B * T, V])."""
    from magma_amd import ops
    R, V = logits.shape
    dev = logits.device
    token = Guarded.of(torch.full((R,), SENTINEL_TOKEN, dtype=I64, device=dev))
    wide = Guarded.of(torch.full((R, V + 5), SENTINEL_F, dtype=F32, device=dev))
    ops.sample_chunk(logits, T, table, count, finish, n_draft=n_draft, history_cols=COLS, warp=warp, out=token.t,
                     filtered=wide.t[:, :V])
    torch.cuda.synchronize()
    assert token.guards_intact() and wide.guards_intact()
    assert bool((wide.t[:, V:] == SENTINEL_F).all()), "written behind a filtered row's V entries"
    return token.t.cpu(), wide.t[:, :V]


def check(got_token, got_filtered, want, R):
    for r in range(R):
        if r in want:
            assert int(got_token[r]) == want[r][0], (r, int(got_token[r]), want[r][0])
            assert torch.equal(got_filtered[r], want[r][1]), f"filtered row {r} differs"
        else:
            assert int(got_token[r]) == SENTINEL_TOKEN and bool((got_filtered[r] == SENTINEL_F).all()), f"skipped row {r} was written"


@pytest.mark.parametrize("warp", [False, True])
@pytest.mark.parametrize("V", [50258, 257])
@pytest.mark.parametrize("B,T", SHAPES)
def test_chunk_selection_is_the_one_row_call(dev, B, T, V, warp):
    g = torch.Generator().manual_seed(B * 100 + T * 10 + V % 7)
    logits = logits_of(B * T, V, dev, seed=B + 3 * T + V)
    rows = records(B, SHAPES.index((B, T)) + 3, warp)
    table = table_of(rows, dev)
    count = torch.randint(1, COLS, (B,), generator=g).to(I32)
    count[0] = 0 if T % 2 == 0 else COLS            # both ends of the range are live
    if B > 1:
        count[1] = COLS if T % 2 == 0 else 0
    n_draft = torch.randint(0, T, (B,), generator=g).to(I32)
    n_draft[B - 1] = T - 1                            # one sequence with every fed row live
    finish = torch.tensor([[-1, 0]] * B, dtype=I32)
    live = [b * T + t for b in range(B) for t in range(int(n_draft[b]) + 1)]
    want = one_row_reference(logits, table, B, T, count, warp, live)
    tok, filt = run_chunk(logits, table, B, T, count.to(dev), n_draft.to(dev), finish.to(dev), warp)
    check(tok, filt, want, B * T)
    sampled = [r for r in live if rows[r // T][0] > 0]
    for r in sampled:
        if rows[r // T][1] > 0:                        # top-k: exactly k survive under the reference's rule, the ties beside them otherwise
            assert int((want[r][1] > -math.inf).sum()) >= rows[r // T][1] and math.isinf(float(want[r][1].min()))
    for r in set(live) - set(sampled):                 # a greedy record: the first maximum alone
        assert want[r][0] == first_max(logits[r]) and int((want[r][1] > -math.inf).sum()) == 1


@pytest.mark.parametrize("warp", [False, True])
@pytest.mark.parametrize("what", ["plain", "n_draft_negative", "n_draft_past", "nan_temperature"])
def test_chunk_skips_the_rows_the_bookkeeping_never_reads(dev, what, warp):
    """A finished sequence, counts outside [0, history_cols] and rows t > n_draft: NaN logits there are never read, the sentinels
    in token and filtered stay, and the live rows are the one-row call's -- also under device values no correct loop leaves."""
    B, T, V = 4, 4, 257
    clean = logits_of(B * T, V, dev, seed=5)
    rows = records(B, 0, warp)
    if what == "nan_temperature":
        rows[0] = (float("nan"),) + rows[0][1:]       # selects greedily (the reference takes the same record)
        rows[1] = (float("inf"),) + rows[1][1:]
    table = table_of(rows, dev)
    for finished, bad_count in ((1, -3), (2, COLS + 1), (3, 2 ** 31 - 1)):
        count = torch.tensor([3, 7, COLS, 0], dtype=I32)
        n_draft = torch.tensor([1, 2, 0, 3], dtype=I32)
        if what == "n_draft_negative":
            n_draft[0] = -5                             # counts as 0
        if what == "n_draft_past":
            n_draft[3], n_draft[1] = T, 2 ** 31 - 1     # count as T - 1
        clamped = n_draft.clamp(0, T - 1)
        finish = torch.tensor([[-1, 0]] * B, dtype=I32)
        finish[finished] = torch.tensor([2, 0x100], dtype=I32)
        dead = (finished + 1) % B
        count[dead] = bad_count
        live = [b * T + t for b in range(B) for t in range(int(clamped[b]) + 1) if b not in (finished, dead)]
        assert live
        logits = clean.clone()
        logits[[r for r in range(B * T) if r not in live]] = float("nan")
        want = one_row_reference(clean, table, B, T, count, warp, live)
        tok, filt = run_chunk(logits, table, B, T, count.to(dev), n_draft.to(dev), finish.to(dev), warp)
        check(tok, filt, want, B * T)
        if what == "nan_temperature" and 0 not in (finished, dead):
            assert want[0][0] == first_max(clean[0])


@pytest.mark.parametrize("warp", [False, True])
def test_the_arming_call_is_the_rows_call_at_counter_zero(dev, warp):
    """T = 1, count = 0, no n_draft: token 0 of every sequence from the prefill logits, as mg_sample_rows_f32 at state[0] = 0."""
    from magma_amd import ops
    B, V = 3, 50258
    logits = logits_of(B, V, dev, seed=9)
    table = table_of(records(B, 0, warp), dev)
    zero, finish = torch.zeros(B, dtype=I32, device=dev), torch.tensor([[-1, 0]] * B, dtype=I32, device=dev)
    want_f = torch.full((B, V), SENTINEL_F, dtype=F32, device=dev)
    want = ops.sample_rows(logits, table, torch.tensor([0, -1], dtype=I32, device=dev), warp, filtered=want_f)
    got_f = torch.full((B, V), SENTINEL_F, dtype=F32, device=dev)
    got = ops.sample_chunk(logits, 1, table, zero, finish, history_cols=COLS, warp=warp, filtered=got_f)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(got_f, want_f)


def test_chunk_refusals_come_before_any_launch(dev):
    from magma_amd import lib as L
    fn = L.load().mg_sample_chunk_f32
    B, T, V = 2, 4, 257
    logits = logits_of(B * T, V, dev, seed=1)
    table = table_of(records(B, 0, True), dev)
    g = Operands(token=Guarded.of(torch.full((B * T,), SENTINEL_TOKEN, dtype=I64, device=dev)),
                 filtered=Guarded.of(torch.full((B * T, V), SENTINEL_F, dtype=F32, device=dev)),
                 count=Guarded.of(torch.zeros(B, dtype=I32, device=dev)), n_draft=Guarded.of(torch.ones(B, dtype=I32, device=dev)),
                 finish=Guarded.of(torch.tensor([[-1, 0]] * B, dtype=I32, device=dev)))
    g.snapshot()
    p = {k: g[k].t.data_ptr() for k in ("token", "filtered", "count", "n_draft", "finish")}

    def call(logits=logits.data_ptr(), ld=logits.stride(0), B=B, T=T, V=V, warp=1, params=table.data_ptr(), count=p["count"],
             n_draft=p["n_draft"], finish=p["finish"], cols=COLS, token=p["token"], filtered=p["filtered"], ldf=V):
        return fn(logits, ld, B, T, V, warp, params, count, n_draft, finish, cols, token, filtered, ldf, None)

    cases = [(dict(T=0), "T"), (dict(T=9), "T"), (dict(B=5), "B * T"), (dict(B=0), "bad logits"), (dict(V=0), "bad logits"),
             (dict(ld=V - 1), "bad logits"), (dict(logits=None), "bad logits"), (dict(warp=2), "warp"), (dict(params=None), "needs"),
             (dict(count=None), "needs"), (dict(finish=None), "needs"), (dict(token=None, filtered=None), "nothing to produce"),
             (dict(ldf=V - 1), "ld_filtered"), (dict(cols=-1), "history_cols"), (dict(params=table.data_ptr() + 8), "16-byte"),
             (dict(count=p["count"] + 2), "4-byte"), (dict(n_draft=p["n_draft"] + 1), "4-byte"), (dict(token=p["token"] + 4), "8-byte")]
    for kw, word in cases:
        rc = call(**kw)
        assert rc != 0 and word in L.load().mg_last_error().decode(), (kw, rc, L.load().mg_last_error().decode())
    g.check("sample_chunk refusals")                    # nothing was launched: the outputs hold their sentinels
    assert call() == 0 and call(n_draft=None, T=1, B=B) == 0
    torch.cuda.synchronize()
    assert all(g[k].guards_intact() for k in p)


# ============================================================================================================ spec_finish_seq
def device_update(st, token, arm, kw):
    from magma_amd import ops
    table = ops.stop_table(kw["eos_ids"], kw["stop_seqs"]).to(token.device)
    ops.spec_finish(st["ids"], st["n_draft"], token, st["history"], st["count"], st["finish"], table, len(kw["eos_ids"]), kw["limit"],
                    st["lookup"], st["lookup_len"], st["stats"], st["state"], kw["num_tokens"], kw["max_ngram"], kw["vocab"], st["pos"],
                    arm=arm, n_seq=len(kw["stop_seqs"]))


def _shape(case):
    return len(case["true"]), case["T"]


@pytest.mark.parametrize("case", NAMED, ids=lambda c: c["name"])
def test_spec_finish_seq_named_cases(dev, case):
    got, stats = run_case(case, device_update, dev)
    assert got == case["want"]
    assert torch.equal(stats, run_case(case)[1])


@pytest.mark.parametrize("B,T", [(1, 2), (2, 8), (4, 4)])
def test_spec_finish_seq_equals_the_host_statement(dev, B, T):
    cases = [c for c in CASES[len(NAMED):] if _shape(c) == (B, T)]
    assert len(cases) == 12
    stops = 0
    for case in cases:
        got, stats = run_case(case, device_update, dev)
        want, want_stats = run_case(case, host_update)
        assert got == want == token_by_token(case), (case, got, want)
        assert torch.equal(stats, want_stats), case
        stops += sum(code >> 8 == 2 for _, _, (_, code) in got)
    assert stops > 0


@pytest.mark.parametrize("B,T", [(1, 2), (2, 8), (4, 4)])
def test_spec_finish_seq_without_sequences_is_spec_finish(dev, B, T):
    """The same inputs through both entry points: every buffer ends with the same bits."""
    from magma_amd import ops
    cols, lcols = 24, 50
    table = ops.stop_table((5, 0, 3), ((1, 2), (4,))).to(dev)       # the sequences are in the table; n_seq = 0 reads none
    for seed in range(8):
        arm = seed >= 6
        st = spec_state(B, T, cols, lcols, seed * 5 + B + T, arm=arm, eos_ids=(5, 0, 3))
        runs = []
        for n_seq in (None, 0):
            d = {k: Guarded.of(v.to(dev)) for k, v in st.items()}
            ops.spec_finish(d["ids"].t, d["n_draft"].t, d["token"].t, d["history"].t, d["count"].t, d["finish"].t, table, 3,
                            (cols, 12)[seed % 2], d["lookup"].t, d["lookup_len"].t, d["stats"].t, d["state"].t, T - 1, 1 + seed % 3, 6,
                            d["pos"].t, arm=arm, n_seq=n_seq)
            torch.cuda.synchronize()
            assert all(v.guards_intact() for v in d.values())
            runs.append({k: v.t.cpu() for k, v in d.items()})
        assert all(torch.equal(runs[0][k], runs[1][k]) for k in st), seed
