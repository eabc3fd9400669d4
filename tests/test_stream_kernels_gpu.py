"""Request streams, the two device entry points (DESIGN.md "Request streams"): the bookkeeping launch of a slot session
(ops.sample_finish_slots) against the host statement (magma_amd.sampling.slot_update, tested on the host by
tests/test_stream_cpu.py) integer for integer over scripted random runs, and the admission launch (ops.slots_admit) against an
indexed copy of clones, its bookkeeping, every refusal, and one case whose target slot lies past 4 GiB."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 10
EOS_IDS = [PAD, 11]
SEQS = [[1, 2], [3], [4, 5, 6], [2, 2], [7, 8, 7, 8]]
FILL = 9                        # in no item
HC, N_STEPS = 32, 100


def _script(B, seed=0):
    """Tokens int64 [B, N_STEPS + 1] over 12 ids (column = the device's step), and the re-admissions: at step s the finished rows
    r with (r + s) % 3 == 0 get a new occupant that begins in column s % HC with a budget of 1 .. 40.  Row 0 of a batch never
    finishes (FILL only, a budget the ring cannot reach) and is never re-admitted."""
    g = torch.Generator().manual_seed(100 + seed)
    tok = torch.randint(0, 12, (B, N_STEPS + 1), generator=g)
    long_rows = torch.arange(B) % 4 == 1          # rows that rarely meet an item: they finish by length
    tok[long_rows] = torch.where(torch.rand(int(long_rows.sum()), N_STEPS + 1, generator=g) < 0.93, torch.tensor(FILL), tok[long_rows])
    limits = torch.randint(1, 41, (B, N_STEPS + 1), generator=g)
    if B > 1:
        tok[0] = FILL
    return tok, limits


def _host_step(tok, ring, step, fin, state, pos, slot, delta):
    """One launch on the host: slot_update is the rule, the rest is the bookkeeping."""
    from magma_amd.sampling import slot_update
    done = fin[:, 0] >= 0
    tok[done] = PAD
    ring[:, step % HC] = tok
    now, why = slot_update(ring, step, done, slot[:, 0], slot[:, 1], EOS_IDS, SEQS)
    new = now & ~done
    fin[new, 0] = step
    fin[new, 1] = why[new, 0] * 256 + why[new, 1]
    pos[~now] += delta          # only rows still open after this step advance
    if bool(now.all()) and int(state[1]) < 0:
        state[1] = step
    state[0] = step + 1
    return new


@pytest.mark.parametrize("B", [1, 5, 16, 300])
def test_finish_slots_equals_host_statement_at_every_step(dev, B):
    from magma_amd import ops
    from magma_amd.sampling import REASON_EOS, REASON_LENGTH, REASON_STOP
    script, limits = _script(B)
    table = ops.stop_table(EOS_IDS, SEQS).to(dev)
    # every buffer inside a larger one filled with a sentinel
    big_h = torch.full((B + 2, HC + 9), -77, dtype=torch.int64, device=dev)
    big_f = torch.full((B + 2, 2), -77, dtype=torch.int32, device=dev)
    big_t = torch.full((B + 2,), -77, dtype=torch.int64, device=dev)
    big_p = torch.full((B + 2,), -77, dtype=torch.int32, device=dev)
    big_s = torch.full((B + 2, 2), -77, dtype=torch.int32, device=dev)
    ring_d, fin_d, tok_d, pos_d, slot_d = big_h[1:B + 1, 4:4 + HC], big_f[1:B + 1], big_t[1:B + 1], big_p[1:B + 1], big_s[1:B + 1]
    ring = torch.full((B, HC), -5, dtype=torch.int64)
    fin = torch.tensor([[-1, 0]] * B, dtype=torch.int64)
    pos = torch.arange(B) * 3 + 11
    slot = torch.stack([torch.ones(B, dtype=torch.int64), limits[:, 0].clone()], 1)     # the session starts at step 1, column 1
    if B > 1:
        slot[0, 1] = 1000
    state = torch.tensor([1, -1])
    ring_d.copy_(ring)
    fin_d.copy_(fin.to(torch.int32))
    pos_d.copy_(pos.to(torch.int32))
    slot_d.copy_(slot.to(torch.int32))
    state_d = state.to(torch.int32).to(dev)
    reasons, latched, frozen_checked = set(), 0, 0
    for step in range(1, N_STEPS + 1):
        if step % 7 == 0:       # new occupants for some finished rows: window, finish record and latch as an admission leaves them
            again = (fin[:, 0] >= 0) & ((torch.arange(B) + step) % 3 == 0)
            if bool(again.any()):
                fin[again] = torch.tensor([-1, 0])
                slot[again, 0], slot[again, 1] = step % HC, limits[again, step]
                state[1] = -1
                fin_d.copy_(fin.to(torch.int32))
                slot_d.copy_(slot.to(torch.int32))
                state_d.copy_(state.to(torch.int32))
        tok = script[:, step].clone()
        tok_d.copy_(tok)
        was_done, pos_before = fin[:, 0] >= 0, pos.clone()
        new = _host_step(tok, ring, step, fin, state, pos, slot, 1)
        ops.sample_finish_slots(tok_d, state_d, table, len(EOS_IDS), len(SEQS), PAD, fin_d, slot_d, ring_d, d_pos=pos_d)
        assert torch.equal(tok_d.cpu(), tok), (step, tok_d.cpu(), tok)
        assert torch.equal(ring_d.cpu(), ring), step
        assert torch.equal(fin_d.cpu().to(torch.int64), fin), (step, fin_d.cpu(), fin)
        assert state_d.tolist() == state.tolist(), (step, state_d, state)
        assert pos_d.tolist() == pos.tolist(), (step, pos_d, pos)
        assert torch.equal(pos_d.cpu()[was_done].to(torch.int64), pos_before[was_done])         # finished rows stay frozen
        frozen_checked += int(was_done.sum())
        reasons |= {int(c) >> 8 for c in fin[new, 1]}
        latched += int(state[1]) == step
    assert frozen_checked > 0
    if B == 1:
        assert latched >= 2                                     # the one row finished, was replaced, finished again
    else:
        assert int(fin[0, 0]) == -1 and int(state[1]) == -1     # the row that never finishes keeps the latch open
        assert reasons == {REASON_EOS, REASON_STOP, REASON_LENGTH}, reasons
    assert N_STEPS > 3 * HC                                     # the ring wrapped three times
    inner = torch.zeros_like(big_h, dtype=torch.bool)
    inner[1:B + 1, 4:4 + HC] = True
    assert bool((big_h[~inner] == -77).all())
    for big in (big_f, big_t, big_p, big_s):
        assert bool((big[0] == -77).all()) and bool((big[-1] == -77).all())


def test_finish_slots_refusals(dev):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    B = 3
    i32 = dict(dtype=torch.int32, device=dev)
    tok, state = torch.zeros(B, dtype=torch.int64, device=dev), torch.tensor([1, -1], **i32)
    fin, slot, pos = torch.zeros(B, 2, **i32), torch.zeros(B, 2, **i32), torch.zeros(B, **i32)
    ring, table = torch.zeros(B, HC, dtype=torch.int64, device=dev), ops.stop_table(EOS_IDS, SEQS).to(dev)
    for n_eos, n_seq in ((0, 0), (9, 0), (1, 17), (1, -1)):
        with pytest.raises(MagmaHipError):
            ops.sample_finish_slots(tok, state, table, n_eos, n_seq, PAD, fin, slot, ring, d_pos=pos)
    assert state.tolist() == [1, -1]


# ---------------------------------------------------------------------------------------------------------------- admission
L_, H_, N_STAGE, S_STAGE, B_, SMAX = 2, 3, 5, 128, 5, 192


def _caches(dev, seed, B=B_, Smax=SMAX, n_stage=N_STAGE, S_stage=S_STAGE):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev)  # noqa: E731
    return mk(L_, n_stage, H_, S_stage, 256), mk(L_, n_stage, H_, S_stage, 256), mk(L_, B, H_, Smax, 256), mk(L_, B, H_, Smax, 256)


def _session_state(dev, B, state0=38):
    i32 = dict(dtype=torch.int32, device=dev)
    return dict(state=torch.tensor([state0, 5], **i32), d_pos=torch.full((B,), 77, **i32),
                token=torch.full((B,), -3, dtype=torch.int64, device=dev), finish=torch.tensor([[2, 0x300]] * B, **i32),
                slot=torch.full((B, 2), -9, **i32), history=torch.full((B, HC), -5, dtype=torch.int64, device=dev))


# (src_row, dst_slot, len, first token, limit) per request, and what the first token leaves in the finish record (None: open)
ADMIT_CASES = {
    "one": ([(3, 2, 65, FILL, 8)], [None]),
    "all": ([(0, 4, 1, FILL, 5), (4, 0, 63, 11, 5), (2, 3, 64, 3, 5), (2, 1, 65, FILL, 1), (1, 2, 7, 1, 2)],
            [None, 0x100 | 1, 0x200 | 1, 0x300, None]),          # open, eos id 1, the one-token sequence, limit 1, open ([1] alone is no item)
}


@pytest.mark.parametrize("case", list(ADMIT_CASES))
def test_slots_admit_equals_indexed_copy(dev, case):
    from magma_amd import ops
    reqs, codes = ADMIT_CASES[case]
    ks, vs, kc, vc = _caches(dev, 3)
    want_k, want_v = kc.clone(), vc.clone()
    st = _session_state(dev, B_)
    before = {k: v.clone() for k, v in st.items()}
    table = ops.stop_table(EOS_IDS, SEQS).to(dev)
    first = torch.tensor([r[3] for r in reqs], dtype=torch.int64, device=dev)
    ops.slots_admit(ks, vs, kc, vc, [r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs], first, [r[4] for r in reqs],
                    st["state"], st["d_pos"], st["token"], st["finish"], st["slot"], st["history"], table, len(EOS_IDS), len(SEQS))
    prev = 37
    c = prev % HC
    for (src, dst, n, t, limit), code in zip(reqs, codes):
        want_k[:, dst, :, :n] = ks[:, src, :, :n]
        want_v[:, dst, :, :n] = vs[:, src, :, :n]
        before["d_pos"][dst], before["token"][dst] = n, t
        before["slot"][dst] = torch.tensor([c, limit], dtype=torch.int32)
        before["history"][dst, c] = t
        before["finish"][dst] = torch.tensor([-1, 0] if code is None else [prev, code], dtype=torch.int32)
    before["state"][1] = -1
    # the whole caches: every other slot, and positions >= len of the target slots, are untouched
    assert torch.equal(kc, want_k) and torch.equal(vc, want_v)
    for name, want in before.items():
        assert torch.equal(st[name], want), (name, st[name], want)


def test_slots_admit_refusals(dev):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    ks, vs, kc, vc = _caches(dev, 4)
    table = ops.stop_table(EOS_IDS, SEQS).to(dev)
    first = torch.full((20,), FILL, dtype=torch.int64, device=dev)

    def refused(kst, vst, kca, vca, src, dst, lens, limits=None):
        B = kca.shape[1]
        st = _session_state(dev, B)
        keep = [t.clone() for t in (kca, vca, *st.values())]
        with pytest.raises(MagmaHipError, match="mg_slots_admit_bf16"):
            ops.slots_admit(kst, vst, kca, vca, src, dst, lens, first, limits or [4] * len(src), st["state"], st["d_pos"], st["token"],
                            st["finish"], st["slot"], st["history"], table, len(EOS_IDS), len(SEQS))
        assert all(torch.equal(a, b) for a, b in zip(keep, (kca, vca, *st.values())))      # refused before anything is launched

    refused(ks, vs, kc, vc, [0, 1], [2, 2], [3, 3])                       # a duplicate slot
    refused(ks, vs, kc, vc, [0], [B_], [3])                               # slot out of range
    refused(ks, vs, kc, vc, [0], [-1], [3])
    refused(ks, vs, kc, vc, [N_STAGE], [0], [3])                          # staging row out of range
    refused(ks, vs, kc, vc, [-1], [0], [3])
    refused(ks, vs, kc, vc, [0], [0], [0])                                # len outside [1, min(S_stage, Smax)]
    refused(ks, vs, kc, vc, [0], [0], [S_STAGE + 1])                      # S_stage < Smax
    refused(kc, vc, ks, vs, [0], [0], [S_STAGE + 1])                      # the roles swapped: Smax < S_stage
    refused(ks, vs, kc, vc, list(range(B_)) + [0], list(range(B_ + 1)), [3] * (B_ + 1))      # n > B
    refused(ks, vs, kc, vc, [], [], [])                                   # n = 0
    big = torch.zeros(1, 17, 1, 8, 256, dtype=torch.bfloat16, device=dev)
    refused(big, big.clone(), big.clone(), big.clone(), [0] * 17, list(range(17)), [1] * 17)   # n above the 16 of one launch
    ops.slots_admit(ks, vs, kc, vc, [0], [0], [S_STAGE], first, [4], *[_session_state(dev, B_)[k] for k in
                    ("state", "d_pos", "token", "finish", "slot", "history")], table, len(EOS_IDS), len(SEQS))     # the bound itself passes


def test_slots_admit_target_slot_past_4_gib(dev):
    """L = 1, H = 1, six slots of 2^21 positions: a slot is 1 GiB, slot 5 begins 5 GiB into each live cache -- past what a 32-bit
    byte offset and a 31-bit element offset hold; with the offset cut to 32 bits the copy would land in slot 1."""
    from magma_amd import ops
    B, Smax, n = 6, 2 ** 21, 65
    need = 2 * B * Smax * 512 + 2 ** 30
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.0f} GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    g = torch.Generator().manual_seed(9)
    ks = torch.randn(1, 2, 1, 128, 256, generator=g).to(torch.bfloat16).to(dev)
    vs = torch.randn(1, 2, 1, 128, 256, generator=g).to(torch.bfloat16).to(dev)
    kc = torch.zeros(1, B, 1, Smax, 256, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros(1, B, 1, Smax, 256, dtype=torch.bfloat16, device=dev)
    assert (kc[0, 5].data_ptr() - kc.data_ptr()) > 2 ** 32
    st = _session_state(dev, B)
    table = ops.stop_table(EOS_IDS, SEQS).to(dev)
    first = torch.tensor([FILL], dtype=torch.int64, device=dev)
    ops.slots_admit(ks, vs, kc, vc, [1], [5], [n], first, [4], st["state"], st["d_pos"], st["token"], st["finish"], st["slot"],
                    st["history"], table, len(EOS_IDS), len(SEQS))
    for cache, stage in ((kc, ks), (vc, vs)):
        assert torch.equal(cache[0, 5, 0, :n], stage[0, 1, 0, :n])
        assert not bool(cache[0, 5, 0, n:n + 64].any())
        for b in range(5):          # slot 1 is where a 32-bit byte offset lands, slot 3 a 31-bit element offset's alias
            assert not bool(cache[0, b, 0, :128].any()), b
    assert int(st["d_pos"][5]) == n and st["finish"][5].tolist() == [-1, 0]
    del kc, vc
    torch.cuda.empty_cache()
