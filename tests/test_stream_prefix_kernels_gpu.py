"""The admission launch behind a session prefix (DESIGN.md "Request streams", session prefix): mg_slots_admit_at_bf16 against an
indexed copy of clones -- the bytes inside [pos0, pos0 + len) are the source's, every other byte of both live caches (NaN patterns
as the fill, compared as int16) is untouched, the bookkeeping is the host restatement --, equal to mg_slots_admit_bf16 at pos0 = 0,
every new refusal, and one case whose target slot lies past 4 GiB."""
import ctypes as C

import pytest
import torch

from test_stream_kernels_gpu import EOS_IDS, FILL, HC, SEQS, _session_state

pytestmark = pytest.mark.gpu

L_, H_, N_STAGE, S_STAGE, B_, SMAX = 2, 2, 5, 128, 5, 192
# (src_row, dst_slot, first token, limit) of up to five requests: neither the slots nor the staging rows are monotone
REQS = [(3, 2, FILL, 5), (0, 4, 11, 5), (4, 0, 3, 5), (2, 3, FILL, 1), (1, 1, 1, 2)]
BOOK = ("state", "d_pos", "token", "finish", "slot", "history")


def first_code(t, limit):
    """What the row test leaves for a first token: an eos id, a one-token stop sequence, the budget, or None (the row is open)."""
    if t in EOS_IDS:
        return 0x100 | EOS_IDS.index(t)
    for i, q in enumerate(SEQS):
        if q == [t]:
            return 0x200 | i
    return 0x300 if limit <= 1 else None


def _bits(dev, seed, *shape):
    """bf16 of random bit patterns: NaNs, infinities and denormals among them."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int16).to(dev).view(torch.bfloat16)


def _caches(dev, seed, B=B_, Smax=SMAX, n_stage=N_STAGE, S_stage=S_STAGE):
    return (_bits(dev, seed, L_, n_stage, H_, S_stage, 256), _bits(dev, seed + 1, L_, n_stage, H_, S_stage, 256),
            _bits(dev, seed + 2, L_, B, H_, Smax, 256), _bits(dev, seed + 3, L_, B, H_, Smax, 256))


def eq16(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def admit_at(ks, vs, kc, vc, src, dst, lens, first, limits, st, table, pos0):
    """The new entry point itself (ops.slots_admit takes the old one at pos0 = 0)."""
    from magma_amd import lib
    n = len(src)
    arr = lambda xs: (C.c_int32 * max(n, 1))(*[int(x) for x in xs])  # noqa: E731
    h = st["history"]
    lib.check(lib.load().mg_slots_admit_at_bf16(
        ks.data_ptr(), vs.data_ptr(), ks.shape[1], ks.shape[3], kc.data_ptr(), vc.data_ptr(), ks.shape[0], kc.shape[1], ks.shape[2],
        kc.shape[3], n, arr(src), arr(dst), arr(lens), first.data_ptr(), arr(limits), st["state"].data_ptr(), st["d_pos"].data_ptr(),
        st["token"].data_ptr(), st["finish"].data_ptr(), st["slot"].data_ptr(), h.data_ptr(), h.stride(0), h.shape[1], table.data_ptr(),
        len(EOS_IDS), len(SEQS), int(pos0), torch.cuda.current_stream().cuda_stream), "mg_slots_admit_at_bf16")


@pytest.fixture(scope="module")
def caches(dev):
    """(kstage, vstage, kcache, vcache): made once, only ever cloned."""
    return _caches(dev, 3)


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("pos0", [0, 1, 31, 64])
def test_admit_at_equals_indexed_copy(dev, caches, pos0, n):
    from magma_amd import ops
    ks, vs, kc0, vc0 = caches
    table = ops.stop_table(EOS_IDS, SEQS).to(dev)
    all_lens = [1, 7, 64, S_STAGE - pos0]
    reqs = REQS[:n]
    first = torch.tensor([r[2] for r in reqs], dtype=torch.int64, device=dev)
    for turn in range(4):                   # every request takes every length once
        lens = [all_lens[(j + turn) % 4] for j in range(n)]
        kc, vc, st = kc0.clone(), vc0.clone(), _session_state(dev, B_)
        want_k, want_v, want = kc0.clone(), vc0.clone(), {k: v.clone() for k, v in st.items()}
        args = (ks, vs, kc, vc, [r[0] for r in reqs], [r[1] for r in reqs], lens, first, [r[3] for r in reqs])
        if pos0 and turn % 2:               # through ops.slots_admit as the session calls it
            ops.slots_admit(*args, *[st[k] for k in BOOK], table, len(EOS_IDS), len(SEQS), pos0=pos0)
        else:
            admit_at(*args, st, table, pos0)
        prev = 37
        c = prev % HC
        for (src, dst, t, limit), m in zip(reqs, lens):
            want_k[:, dst, :, pos0:pos0 + m] = ks[:, src, :, pos0:pos0 + m]
            want_v[:, dst, :, pos0:pos0 + m] = vs[:, src, :, pos0:pos0 + m]
            code = first_code(t, limit)
            want["d_pos"][dst], want["token"][dst] = pos0 + m, t
            want["slot"][dst] = torch.tensor([c, limit], dtype=torch.int32)
            want["history"][dst, c] = t
            want["finish"][dst] = torch.tensor([-1, 0] if code is None else [prev, code], dtype=torch.int32)
        want["state"][1] = -1
        # the whole caches, bit for bit: the range is the source's, everything else -- the prefix region [0, pos0) of the target
        # slots, their positions past pos0 + len, every other slot -- is what it was
        assert eq16(kc, want_k) and eq16(vc, want_v), (pos0, lens)
        assert not eq16(kc, kc0) and not eq16(vc, vc0)
        for name in BOOK:
            assert torch.equal(st[name], want[name]), (name, pos0, lens, st[name], want[name])
        if pos0 == 0:                       # the old entry point on clones: the same bytes and the same bookkeeping
            kc1, vc1, st1 = kc0.clone(), vc0.clone(), _session_state(dev, B_)
            ops.slots_admit(ks, vs, kc1, vc1, *args[4:], *[st1[k] for k in BOOK], table, len(EOS_IDS), len(SEQS))
            assert eq16(kc1, kc) and eq16(vc1, vc) and all(torch.equal(st1[k], st[k]) for k in BOOK)
    assert {first_code(r[2], r[3]) for r in REQS} == {None, 0x100 | 1, 0x200 | 1, 0x300}


def test_admit_at_refusals(dev, caches):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    ks, vs, kc0, vc0 = caches
    table = ops.stop_table(EOS_IDS, SEQS).to(dev)
    first = torch.full((8,), FILL, dtype=torch.int64, device=dev)

    def refused(kst, vst, kca, vca, lens, pos0, through_ops=False):
        kca, vca = kca.clone(), vca.clone()
        st = _session_state(dev, kca.shape[1])
        keep = [t.clone() for t in (kca, vca, *st.values())]
        src, dst = list(range(len(lens))), list(range(len(lens)))[::-1]
        with pytest.raises(MagmaHipError, match="mg_slots_admit_at_bf16"):
            if through_ops:
                ops.slots_admit(kst, vst, kca, vca, src, dst, lens, first, [4] * len(lens), *[st[k] for k in BOOK], table, len(EOS_IDS),
                                len(SEQS), pos0=pos0)
            else:
                admit_at(kst, vst, kca, vca, src, dst, lens, first, [4] * len(lens), st, table, pos0)
        assert all(eq16(a, b) if a.dtype == torch.bfloat16 else torch.equal(a, b) for a, b in zip(keep, (kca, vca, *st.values())))

    refused(ks, vs, kc0, vc0, [3], -1)                                    # pos0 < 0
    refused(ks, vs, kc0, vc0, [3], -1, through_ops=True)
    refused(ks, vs, kc0, vc0, [3, 0], 5)                                  # len < 1
    refused(ks, vs, kc0, vc0, [3, -2], 5)
    refused(ks, vs, kc0, vc0, [3, S_STAGE - 31 + 1], 31)                  # pos0 + len > S_stage < Smax
    refused(ks, vs, kc0, vc0, [S_STAGE - 31 + 1], 31, through_ops=True)
    refused(kc0, vc0, ks, vs, [3, S_STAGE - 31 + 1], 31)                  # the roles swapped: pos0 + len > Smax < S_stage
    refused(ks, vs, kc0, vc0, [1], S_STAGE)                               # no position left behind pos0
    refused(ks, vs, kc0, vc0, [1], 2 ** 31 - 1)                           # pos0 + len does not wrap
    kc, vc, st = kc0.clone(), vc0.clone(), _session_state(dev, B_)
    admit_at(ks, vs, kc, vc, [0], [0], [S_STAGE - 31], first, [4], st, table, 31)             # the bound itself passes
    assert int(st["d_pos"][0]) == S_STAGE and eq16(kc[:, 0, :, 31:S_STAGE], ks[:, 0, :, 31:])


def test_admit_at_target_slot_past_4_gib(dev):
    """L = 1, H = 1, six slots of 2^21 positions: a slot is 1 GiB, slot 5 begins 5 GiB into each live cache -- past what a 32-bit
    byte offset and a 31-bit element offset hold; with the offset cut to 32 bits the copy would land in slot 1."""
    from magma_amd import ops
    B, Smax, pos0, n = 6, 2 ** 21, 37, 65
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
    ops.slots_admit(ks, vs, kc, vc, [1], [5], [n], first, [4], *[st[k] for k in BOOK], table, len(EOS_IDS), len(SEQS), pos0=pos0)
    for cache, stage in ((kc, ks), (vc, vs)):
        assert torch.equal(cache[0, 5, 0, pos0:pos0 + n], stage[0, 1, 0, pos0:pos0 + n])
        assert not bool(cache[0, 5, 0, :pos0].any()) and not bool(cache[0, 5, 0, pos0 + n:pos0 + n + 64].any())
        for b in range(5):          # slot 1 is where a 32-bit byte offset lands, slot 3 a 31-bit element offset's alias
            assert not bool(cache[0, b, 0, :128].any()), b
    assert int(st["d_pos"][5]) == pos0 + n and st["finish"][5].tolist() == [-1, 0]
    del kc, vc
    torch.cuda.empty_cache()
