"""The contrastive-search kernels (DESIGN.md "Contrastive search"; ABI 22) one by one: mg_contrastive_topk_f32 against a sort,
mg_contrastive_sim_bf16 + mg_contrastive_finish against the host statement contrastive_rank per element under the derived
bound (tests/contrastive_cases.py), mg_kv_broadcast_bf16 against a clone, and what the launches refuse."""
import pytest
import torch

import contrastive_cases as CC
from group_beam_cases import gapped_logits

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- the top-k
@pytest.mark.parametrize("V", [64, 1056, 50258])
@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_topk_against_a_sort(dev, V, k):
    from magma_amd import ops
    B, R, ld = 3, 3 * k, V + 7
    x = gapped_logits(R, V, seed=V + k)
    src = torch.tensor([b * k + (k - 1) for b in range(B)], dtype=torch.int32)      # not the first row of a group (k > 1)
    dup = int(src[1])                           # exact duplicates at the top of one row: a tie goes to the smaller id
    top = float(x[dup].max()) + 1.0
    x[dup, torch.tensor([V - 1, 3, V // 2, 7, 11])] = top
    xd = torch.full((R, ld), 1e30, device=dev)                                       # guard columns that would win, were they read
    xd[:, :V] = x.to(dev)
    token = torch.full((R + 4,), -7, dtype=torch.int64, device=dev)
    cand_p = torch.full((B * k + 4,), -7.0, device=dev)
    ops.contrastive_topk(xd[:, :V], src.to(dev), k, token[:R], cand_p[: B * k])
    p = torch.softmax(x[src.long()].double(), -1)
    order = torch.sort(-p, dim=-1, stable=True).indices[:, :k]                        # (-p, id) ascending
    assert torch.equal(token[:R].cpu().view(B, k), order)
    assert sorted(order[1, : min(k, 5)].tolist()) == sorted([3, 7, 11, V // 2, V - 1])[: min(k, 5)]
    err = (cand_p[: B * k].cpu().double().view(B, k) - torch.take_along_dim(p, order, 1)).abs().max()
    print(f"V {V} k {k}: max |dp| {float(err):.3e}")
    assert float(err) <= CC.P_BOUND
    assert bool((token[R:] == -7).all()) and bool((cand_p[B * k:] == -7.0).all())
    assert bool((xd[:, V:] == 1e30).all())


# ------------------------------------------------------------------------------------------------- similarity and selection
def _device_step(dev, case, eos=5, tokens=None, state=None, uniform_pos=False):
    """One sim + finish on a case's inputs; returns every buffer the two launches touch."""
    from magma_amd import ops
    ctx, hidden = case["ctx"].to(dev), case["hidden"].to(dev)
    B, Tmax, d = ctx.shape
    k = case["k"]
    R = B * k
    o = dict(ctx=ctx, ctx0=ctx.clone(), hidden=hidden.view(R, d).contiguous(), ctx_len=case["ctx_len"].to(dev),
             part=torch.full((B, ops.contrastive_chunks(Tmax), k), 7.0, device=dev), cand_p=case["p"].to(dev).contiguous(),
             src=torch.full((B,), -1, dtype=torch.int32, device=dev),
             token=(torch.arange(R, dtype=torch.int64) * 3 + 11 if tokens is None else tokens).to(dev),
             history=torch.full((R, 6), -1, dtype=torch.int64, device=dev),
             state=torch.tensor([2, -1] if state is None else state, dtype=torch.int32, device=dev),
             d_pos=(torch.tensor([9], dtype=torch.int32) if uniform_pos else torch.arange(R, dtype=torch.int32) + 4).to(dev))
    len_max = int(case["ctx_len"].max())
    ops.contrastive_sim(o["hidden"], ctx, o["ctx_len"], k, o["part"], len_max)
    ops.contrastive_finish(o["part"], o["cand_p"], case["alpha"], o["hidden"], ctx, o["ctx_len"], o["src"], o["token"], eos,
                           o["state"], len_max, d_pos=o["d_pos"], history=o["history"], pos_stride=0 if uniform_pos else 1)
    return o


@pytest.mark.parametrize("d,k,T,adv", CC.kernel_cases())
def test_sim_and_finish_against_host_statement(dev, d, k, T, adv):
    case = CC.sim_case(d, k, T, CC.case_seed(d, k, T, adv), adversarial=adv)
    sel, score, pen, gap = CC.reference(case)
    assert float(gap.min()) > CC.gap_bound(case["alpha"], d)                       # decided, asserted, never skipped
    o = _device_step(dev, case)
    B, lens = case["ctx"].shape[0], case["ctx_len"].long()
    part = o["part"].cpu()
    # per chunk: a chunk with a valid position holds that chunk's maximum, any other the sentinel
    chunks = part.shape[1]
    for b in range(B):
        for c in range(chunks):
            lo, hi = c * CC.CHUNK, min((c + 1) * CC.CHUNK, int(lens[b]))
            if hi <= lo:
                assert bool((part[b, c] == -1e30).all()), (b, c)
            else:
                one = dict(case, ctx=case["ctx"][b: b + 1, lo:hi], ctx_len=torch.tensor([hi - lo]), hidden=case["hidden"][b: b + 1],
                           p=case["p"][b: b + 1])
                ref = CC.reference(one)[2][0]
                assert float((part[b, c].double() - ref).abs().max()) <= CC.cos_bound(d), (b, c)
    got_pen = part.max(1).values.double()
    err = float((got_pen - pen).abs().max())
    print(f"d {d} k {k} T {T} {adv}: max |dcos| {err:.3e} (bound {CC.cos_bound(d):.3e}), smallest gap {float(gap.min()):.3e}")
    assert err <= CC.cos_bound(d)
    R = B * k
    rows = torch.arange(B) * k + sel
    assert torch.equal(o["src"].cpu().long(), rows)
    # the context store: the selected hidden row appended bit for bit, nothing else touched
    ctx, ctx0 = o["ctx"].cpu(), o["ctx0"].cpu()
    for b in range(B):
        assert torch.equal(ctx[b, lens[b]], case["hidden"][b, sel[b]])
        ctx0[b, lens[b]] = case["hidden"][b, sel[b]]
    assert torch.equal(ctx.view(torch.int16), ctx0.view(torch.int16))
    assert torch.equal(o["ctx_len"].cpu().long(), lens + 1)
    # the bookkeeping: the selected token in column `step` of the sample's k history rows, step + 1, no eos, every row advanced
    tok = (rows * 3 + 11)
    hist = torch.full((R, 6), -1, dtype=torch.int64)
    hist[:, 2] = tok.repeat_interleave(k)
    assert torch.equal(o["history"].cpu(), hist)
    assert o["state"].cpu().tolist() == [3, -1]
    assert torch.equal(o["d_pos"].cpu().long(), torch.arange(R) + 5)
    assert torch.equal(o["token"].cpu(), torch.arange(R, dtype=torch.int64) * 3 + 11)


def test_finish_with_one_shared_position(dev):
    case = CC.sim_case(512, 5, 33, 77)
    o = _device_step(dev, case, uniform_pos=True)
    assert o["d_pos"].cpu().tolist() == [10]
    assert torch.equal(o["src"].cpu().long(), torch.arange(3) * 5 + CC.reference(case)[0])


def test_eos_latch_fires_when_every_sample_emits_eos(dev):
    """A scripted run of five steps: candidate 0 is selected every time (its probability dominates), candidate 1 of every sample holds
    eos throughout and must not count.  Samples emit eos at steps {1, 3}, {3}, {2, 3}: the latch records step 3 and stays."""
    from magma_amd import ops
    eos, B, k, d, Tmax = 5, 3, 2, 256, 64
    g = torch.Generator().manual_seed(3)
    ctx = torch.randn(B, Tmax, d, generator=g).to(BF16).to(dev)
    ctx_len = torch.tensor([3, 1, 2], dtype=torch.int32, device=dev)
    cand_p = torch.tensor([[0.9, 0.05]] * B, device=dev)
    part = torch.zeros(B, ops.contrastive_chunks(Tmax), k, device=dev)
    src = torch.zeros(B, dtype=torch.int32, device=dev)
    state = torch.tensor([0, -1], dtype=torch.int32, device=dev)
    history = torch.zeros(B * k, 8, dtype=torch.int64, device=dev)
    script = {0: (1, 3), 1: (3,), 2: (2, 3)}
    for step in range(5):
        hidden = torch.randn(B * k, d, generator=g).to(BF16).to(dev)
        token = torch.tensor([[eos if step in script[b] else 20 + step + b, eos] for b in range(B)], dtype=torch.int64, device=dev).view(-1)
        ops.contrastive_sim(hidden, ctx, ctx_len, k, part, 3 + step)
        ops.contrastive_finish(part, cand_p, 0.1, hidden, ctx, ctx_len, src, token, eos, state, 3 + step, history=history)
        assert state.cpu().tolist() == [step + 1, 3 if step >= 3 else -1], step
        assert src.cpu().tolist() == [0, 2, 4]
    assert ctx_len.cpu().tolist() == [8, 6, 7]
    assert history[::k, :5].cpu().tolist() == [[eos if s in script[b] else 20 + s + b for s in range(5)] for b in range(B)]
    assert torch.equal(history[::k], history[1::k])


# ------------------------------------------------------------------------------------------------------- the K / V broadcast
@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("mode", ["after_advance", "before_advance", "shared"])
def test_kv_broadcast(dev, H, mode):
    from magma_amd import ops
    L, R, k, Smax = 2, 6, 3, 40
    g = torch.Generator().manual_seed(H)
    kc = torch.randn(L, R, H, Smax, 256, generator=g).to(BF16).to(dev)
    vc = torch.randn(L, R, H, Smax, 256, generator=g).to(BF16).to(dev)
    k0, v0 = kc.clone(), vc.clone()
    src = torch.tensor([1, 5], dtype=torch.int32, device=dev)
    if mode == "after_advance":              # positions 0 and Smax - 1, read one behind the advanced write position
        pos, d_pos, kw = [0, Smax - 1], torch.tensor([1] * 3 + [Smax] * 3, dtype=torch.int32), dict(pos_stride=1, pos_delta=-1)
    elif mode == "before_advance":
        pos, d_pos, kw = [5, 17], torch.tensor([5] * 3 + [17] * 3, dtype=torch.int32), dict(pos_stride=1)
    else:                                    # one position for the batch
        pos, d_pos, kw = [8, 8], torch.tensor([9], dtype=torch.int32), dict(pos_stride=0, pos_delta=-1)
    ops.kv_broadcast(kc, vc, k, src, d_pos.to(dev), **kw)
    for b in range(2):
        s = int(src[b])
        for r in range(b * k, b * k + k):
            assert torch.equal(kc[:, r, :, pos[b]], k0[:, s, :, pos[b]]) and torch.equal(vc[:, r, :, pos[b]], v0[:, s, :, pos[b]])
            k0[:, r, :, pos[b]], v0[:, r, :, pos[b]] = k0[:, s, :, pos[b]].clone(), v0[:, s, :, pos[b]].clone()
    assert torch.equal(kc.view(torch.int16), k0.view(torch.int16)) and torch.equal(vc.view(torch.int16), v0.view(torch.int16))
    # a group of one row has no sibling; a source outside the group or a position outside the cache copies nothing
    ops.kv_broadcast(kc, vc, 1, torch.arange(R, dtype=torch.int32, device=dev), torch.full((R,), 3, dtype=torch.int32, device=dev),
                     pos_stride=1)
    ops.kv_broadcast(kc, vc, k, torch.tensor([4, 1], dtype=torch.int32, device=dev), d_pos.to(dev), **kw)
    ops.kv_broadcast(kc, vc, k, src, torch.full((R,), Smax + 1, dtype=torch.int32, device=dev), pos_stride=1)
    ops.kv_broadcast(kc, vc, k, src, torch.zeros(R, dtype=torch.int32, device=dev), pos_stride=1, pos_delta=-1)
    assert torch.equal(kc.view(torch.int16), k0.view(torch.int16)) and torch.equal(vc.view(torch.int16), v0.view(torch.int16))


# --------------------------------------------------------------------------------------------------------- what is refused
def test_launch_validation(dev):
    from magma_amd import ops
    from magma_amd.lib import MagmaHipError
    B, k, d, Tmax = 2, 4, 512, 64
    n_chunk = ops.contrastive_chunks(Tmax)

    def bufs(k=k, d=d):
        return dict(hidden=torch.ones(B * k + 1, d, dtype=BF16, device=dev), ctx=torch.ones(B, Tmax, d, dtype=BF16, device=dev),
                    ctx_len=torch.full((B,), 3, dtype=torch.int32, device=dev), part=torch.full((B * n_chunk * k,), 7.0, device=dev),
                    cand_p=torch.full((B, k), 0.1, device=dev), src=torch.full((B,), -1, dtype=torch.int32, device=dev),
                    token=torch.full((B * k,), 9, dtype=torch.int64, device=dev),
                    state=torch.tensor([0, -1], dtype=torch.int32, device=dev))

    def untouched(o, k=k):
        assert bool((o["part"] == 7.0).all()) and bool((o["src"] == -1).all()) and o["state"].cpu().tolist() == [0, -1]
        assert bool((o["ctx"] == 1).all()) and o["ctx_len"].cpu().tolist() == [3] * B and bool((o["token"] == 9).all())

    def sim(o, k=k, len_max=3, hidden=None):
        ops.contrastive_sim(o["hidden"][: B * k] if hidden is None else hidden, o["ctx"], o["ctx_len"], k, o["part"], len_max)

    def finish(o, k=k, alpha=0.6, len_max=3, hidden=None):
        ops.contrastive_finish(o["part"], o["cand_p"], alpha, o["hidden"][: B * k] if hidden is None else hidden, o["ctx"],
                               o["ctx_len"], o["src"], o["token"], 5, o["state"], len_max)

    o = bufs()
    sim(o)
    finish(o)                                                             # the well-formed launches pass
    assert o["state"].cpu().tolist() == [1, -1]
    o = bufs()
    shifted = o["hidden"].view(-1)[4: 4 + B * k * d].view(B * k, d)       # 8 bytes off a 16-byte boundary
    for call in (lambda: sim(o, hidden=shifted), lambda: finish(o, hidden=shifted),
                 lambda: sim(o, len_max=Tmax + 1), lambda: finish(o, len_max=Tmax),
                 lambda: finish(o, alpha=0.0), lambda: finish(o, alpha=1.5), lambda: finish(o, alpha=float("nan")),
                 lambda: finish(o, alpha=-0.1)):
        with pytest.raises(MagmaHipError):
            call()
    untouched(o)
    for bad_k in (0, 17):
        o = bufs(k=bad_k)
        with pytest.raises(MagmaHipError):
            sim(o, k=bad_k)
        with pytest.raises(MagmaHipError):
            finish(o, k=bad_k)
        with pytest.raises(MagmaHipError):
            ops.contrastive_topk(torch.zeros(B * bad_k, 64, device=dev), o["src"], bad_k, o["token"], o["cand_p"].view(-1))
        untouched(o, bad_k)
    o = bufs(d=384)                                                       # d must be a multiple of 256
    with pytest.raises(MagmaHipError):
        sim(o)
    with pytest.raises(MagmaHipError):
        finish(o)
    untouched(o)
    with pytest.raises(MagmaHipError):                                    # more candidates than tokens
        ops.contrastive_topk(torch.zeros(B * k, 3, device=dev), o["src"], k, o["token"], o["cand_p"].view(-1))
    kc = torch.zeros(1, 6, 1, 8, 256, dtype=BF16, device=dev)
    d_pos = torch.zeros(6, dtype=torch.int32, device=dev)
    for bad_k in (0, 4, 17):                                              # k must divide the rows
        with pytest.raises((MagmaHipError, AssertionError)):
            ops.kv_broadcast(kc, kc.clone(), bad_k, torch.zeros(2, dtype=torch.int32, device=dev), d_pos, pos_stride=1)
