"""Ranking choices (ABI 19; DESIGN.md "Ranking choices"), the kernels:

  * mg_attn_prefill_tree_bf16 -- a chunk whose rows are the nodes of a trie in preorder, query t sees the cache below p_b and the
    chunk keys j <= t < sub[b][j] -- bit for bit the cached-chunk kernel on a chain, and against an fp32 PyTorch statement and
    the per-element bound of the cached-chunk kernel on general trees;
  * mg_rotary_split_at_bf16: the slot and the angle apart; off[s] = s is mg_rotary_split_bf16 with pos_stride = 1;
  * mg_token_logprobs_rows_f32: mg_token_logprobs_f32 with a row indirection, the same bits."""
import math
import random

import pytest
import torch

import kernel_compare as kcmp
from magma_amd.sampling import TokenTrie

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B, H, SMAX = 3, 2, 384
POS = (1, 37, 190)
MG_ERR_SHAPE = -1


def rnd(*shape, dev, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def rel(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-12))


def operands(T, dev, seed=0, Smax=SMAX, rows=B):
    kc = rnd(rows, H, Smax, 256, dev=dev, seed=seed + 1, scale=0.5).to(BF16)
    vc = rnd(rows, H, Smax, 256, dev=dev, seed=seed + 2).to(BF16)
    q = rnd(rows, H, T, 256, dev=dev, seed=seed + 3, scale=0.5).to(BF16)
    return q, kc, vc


# ------------------------------------------------------------------------------------------------------------ the trees
def sub_of_depths(depth):
    """sub of a preorder depth list: the first later row that is no deeper, or N."""
    N = len(depth)
    return [next((j for j in range(i + 1, N) if depth[j] <= depth[i]), N) for i in range(N)]


def star(n):
    return list(range(1, n + 1))


def binary_tree(levels):
    seqs = [[(c >> k) & 1 for k in range(levels)] for c in range(2 ** levels)]
    return TokenTrie(seqs).rows().sub.tolist()            # 2 + 4 + ... + 2^levels nodes


def random_tree(n, seed):
    """Preorder depths by a random walk: deeper by one, or back to any shallower level.  Two long spines are planted so that
    subtrees straddle the 32-key tile edges and the 128-query block edge."""
    rng = random.Random(seed)
    depth = [0]
    for i in range(1, n):
        if i in range(20, 45) or i in range(100, n):         # a spine across keys 32 and one across 128
            depth.append(depth[-1] + 1 if rng.random() < 0.8 else depth[-1])
        else:
            depth.append(rng.randint(0, depth[-1] + 1))
    return sub_of_depths(depth)


def pad_sub(subs, T):
    out = (torch.arange(T, dtype=torch.int32) + 1).repeat(len(subs), 1)
    for b, s in enumerate(subs):
        out[b, : len(s)] = torch.tensor(s, dtype=torch.int32)
    return out


def tree_mask(sub, pos, Sk):
    """[B, 1, T, Sk] bool, the statement of the mask: query t of row b sees the cache keys [0, p_b) and the chunk key j (slot
    p_b + j) iff j <= t < sub[b][j]."""
    Bn, T = sub.shape
    mask = torch.zeros(Bn, 1, T, Sk, dtype=torch.bool)
    t, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    for b, p in enumerate(pos):
        mask[b, 0, :, :p] = True
        mask[b, 0, :, p:p + T] = (j <= t) & (t < sub[b].to(torch.int64)[None, :])
    return mask


def ref_tree(q, kc, vc, mask_b):
    """fp32 statement of one row: q (H, T, 256), mask_b (1, T, Sk)."""
    sc = q.float().cpu() @ kc.float().cpu().transpose(-1, -2) / 16.0
    sc = sc.masked_fill(~mask_b, float("-inf"))
    return (torch.softmax(sc, -1) @ vc.float().cpu()).transpose(0, 1).reshape(q.shape[1], -1)


def assert_tree_attention(out, q, kc, vc, sub, pos, what):
    """Per element, in the manner of kernel_compare.assert_causal_attention: the cached-chunk kernel's bound (the same arithmetic:
    bf16 P, one possible rescale per 32-key tile over p + T keys) under the tree mask."""
    T = q.shape[2]
    mask = tree_mask(sub.cpu(), pos, kc.shape[2]).to(q.device)
    terms = kcmp.attention_terms(q, kc, vc, mask)
    bound = kcmp.attention_bound(terms, max(pos) + T, out.dtype, K=256)
    return kcmp.assert_elementwise(out, kcmp.rows_of(terms["ref"]), kcmp.rows_of(bound), what)


def run_tree(q, kc, vc, sub, pos, dev):
    from magma_amd import ops
    T = q.shape[2]
    out = torch.full((q.shape[0] * T, H * 256), float("nan"), dtype=BF16, device=dev)
    ops.attn_prefill_tree(q, kc, vc, out, q.shape[0], H, T, torch.tensor(pos, dtype=torch.int32, device=dev), sub.to(dev),
                          p_min=min(pos), pos_stride=1)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("T", [1, 5, 32, 33, 130])
def test_chain_gives_the_bytes_of_the_cached_chunk_kernel(dev, T):
    from magma_amd import ops
    q, kc, vc = operands(T, dev)
    sub = torch.full((B, T), T, dtype=torch.int32)
    got = run_tree(q, kc, vc, sub, POS, dev)
    ref = torch.full_like(got, float("nan"))
    ops.attn_prefill_cached(q, kc, vc, ref, B, H, T, torch.tensor(POS, dtype=torch.int32, device=dev), pos_stride=1)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), f"T = {T}: {(got != ref).sum().item()} elements differ"
    # one shared position (pos_stride 0) reads d_pos[0] for every row
    out0, ref0 = torch.empty_like(got), torch.empty_like(got)
    d0 = torch.tensor([37], dtype=torch.int32, device=dev)
    ops.attn_prefill_tree(q, kc, vc, out0, B, H, T, d0, sub.to(dev), p_min=37, pos_stride=0)
    ops.attn_prefill_cached(q, kc, vc, ref0, B, H, T, d0, pos_stride=0)
    assert torch.equal(out0.view(torch.int16), ref0.view(torch.int16))


TREES = {
    "star33": lambda: [star(33)] * B,
    "binary5": lambda: [binary_tree(5)] * B,
    "random130": lambda: [random_tree(130, seed) for seed in (1, 2, 3)],
    "ragged": lambda: [star(1), random_tree(40, 4), random_tree(130, 5)],
}


def test_the_random_trees_straddle_tile_and_block_edges():
    for seed in (1, 2, 3, 5):
        sub = random_tree(130, seed)
        assert any(j < 32 < s for j, s in enumerate(sub)) and any(j < 128 < s for j, s in enumerate(sub)), seed
        assert any(s == j + 1 for j, s in enumerate(sub)) and len(set(sub)) > 20, seed
    assert len(binary_tree(5)) == 62


@pytest.mark.parametrize("tree", sorted(TREES))
def test_general_trees_against_the_fp32_statement(dev, tree):
    subs = TREES[tree]()
    T = max(len(s) for s in subs)
    sub = pad_sub(subs, T)
    q, kc, vc = operands(T, dev, seed=10)
    out = run_tree(q, kc, vc, sub, POS, dev)
    mask = tree_mask(sub, POS, SMAX)
    for b in range(B):
        e = rel(out[b * T:(b + 1) * T], ref_tree(q[b], kc[b], vc[b], mask[b]))
        assert math.isfinite(e) and e <= 3e-3, f"{tree}, row {b} (p = {POS[b]}): rel-L2 {e:.3e}"
    assert_tree_attention(out, q, kc, vc, sub, POS, f"tree attention, {tree}")


@pytest.mark.parametrize("plant", ["own slot", "first row outside a subtree"])
@pytest.mark.parametrize("tree", ["binary5", "random130"])
def test_the_mask_counts(dev, tree, plant):
    """Keys that make both compares of j <= t < sub[j] count.  "own slot": k[t] = bf16(2 q[t] + 0.25 noise) dominates row t, the
    only new key a leaf sees -- a first compare that is off by one (j < t) loses it.  "first row outside a subtree": the key in
    slot j is 4 q[sub[j]], the query of the first row that is NOT below node j -- a second compare that is off by one
    (t <= sub[j]) lets it dominate that row.  Either moves the rows far outside the per-element bound."""
    subs = TREES[tree]()
    T = max(len(s) for s in subs)
    sub = pad_sub(subs, T)
    q, kc, vc = operands(T, dev, seed=20)
    noise = rnd(B, H, T, 256, dev=dev, seed=24, scale=0.25)
    planted = 0
    for b, p in enumerate(POS):
        if plant == "own slot":
            kc[b, :, p:p + T] = (2.0 * q[b].float() + noise[b]).to(BF16)
            planted += T
        else:
            js = [j for j in range(T) if int(sub[b, j]) < T]
            kc[b, :, [p + j for j in js]] = (q[b, :, [int(sub[b, j]) for j in js]].float() * 4).to(BF16)
            planted += len(js)
    assert planted > T
    out = run_tree(q, kc, vc, sub, POS, dev)
    assert_tree_attention(out, q, kc, vc, sub, POS, f"tree attention, {tree}, {plant}")
    mask = tree_mask(sub, POS, SMAX)
    for b in range(B):
        assert rel(out[b * T:(b + 1) * T], ref_tree(q[b], kc[b], vc[b], mask[b])) <= 3e-3
    # the statement itself sees the plant: with the compare off by one the reference moves by far more than the bound
    wrong = mask.clone()
    t, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    for b, p in enumerate(POS):
        s = sub[b].to(torch.int64)[None, :]
        wrong[b, 0, :, p:p + T] = ((j < t) & (t < s)) if plant == "own slot" else ((j <= t) & (t <= s))
    moved = max(rel(ref_tree(q[b], kc[b], vc[b], wrong[b]), ref_tree(q[b], kc[b], vc[b], mask[b])) for b in range(B))
    assert moved > 0.1, moved


def test_tree_attention_refusals(dev):
    """p_b = 0, sub missing, a misaligned stride: the error code, and nothing launched (out keeps its bytes)."""
    from magma_amd import lib, ops
    T = 4
    q, kc, vc = operands(T, dev, Smax=64)
    out = torch.full((B * T, H * 256), 7.0, dtype=BF16, device=dev)
    d_pos = torch.tensor([0, 3, 5], dtype=torch.int32, device=dev)
    sub = torch.full((B, T), T, dtype=torch.int32, device=dev)
    dll = lib.load()

    def call(q_ld=256, q_sb=H * T * 256, q_sh=T * 256, sub_p=sub.data_ptr(), p_min=3):
        return dll.mg_attn_prefill_tree_bf16(q.data_ptr(), q_ld, q_sb, q_sh, kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H * 256,
                                             B, H, T, 64, d_pos.data_ptr(), 1, sub_p, p_min, None)
    assert call(p_min=0) == MG_ERR_SHAPE and b"cached key" in dll.mg_last_error()
    assert call(sub_p=None) == MG_ERR_SHAPE and b"sub" in dll.mg_last_error()
    assert call(q_ld=260) == MG_ERR_SHAPE and call(q_sh=T * 256 + 4) == MG_ERR_SHAPE and call(q_sb=-8) == MG_ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(lib.MagmaHipError):
        ops.attn_prefill_tree(q, kc, vc, out, B, H, T, d_pos, sub, p_min=0, pos_stride=1)
    with pytest.raises(lib.MagmaHipError):
        ops.attn_prefill_tree(q, kc, vc, out, B, H, T, d_pos, None, p_min=3, pos_stride=1)
    with pytest.raises(ValueError):
        ops.attn_prefill_tree(q, kc, vc, out, B, H, T, d_pos, sub[:, :2].contiguous(), p_min=3, pos_stride=1)
    with pytest.raises(ValueError):
        ops.attn_prefill_tree(q, kc, vc, out, B, H, T, d_pos, sub.to(torch.int64), p_min=3, pos_stride=1)
    assert bool((out == 7.0).all())


# --------------------------------------------------------------------------------------------------------------- rotary
def rotary_operands(dev, T, rot=64, Smax=256):
    from oracle.model import rotary_tables
    d = H * 256
    kc0 = rnd(B, H, Smax, 256, dev=dev, seed=11, scale=0.5).to(BF16)
    vc0 = rnd(B, H, Smax, 256, dev=dev, seed=12).to(BF16)
    qkv = rnd(B * T, 3 * d, dev=dev, seed=13, scale=0.5).to(BF16)
    sin_t, cos_t = rotary_tables(rot, Smax)
    return kc0, vc0, qkv, sin_t.to(dev).contiguous(), cos_t.to(dev).contiguous()


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("T", [6, 33, 70])
def test_rotary_at_own_offsets_gives_the_bytes_of_the_chunk_rotary(dev, T):
    from magma_amd import ops
    rot, Smax = 64, 256
    kc0, vc0, qkv, sin_t, cos_t = rotary_operands(dev, T, rot, Smax)
    d_pos = torch.tensor(POS, dtype=torch.int32, device=dev)           # row 2 (p = 190) runs past Smax at T = 70: skipped slots
    off = torch.arange(T, dtype=torch.int32, device=dev).repeat(B, 1)
    kc, vc, kr, vr = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
    q, qr = (torch.full((B, H, T, 256), 3.0, dtype=BF16, device=dev) for _ in range(2))
    ops.rotary_split_at(qkv, B, T, H, rot, sin_t, cos_t, q, kc, vc, d_pos, off)
    ops.rotary_split(qkv, B, T, H, rot, sin_t, cos_t, qr, kr, vr, d_pos=d_pos, pos_stride=1)
    torch.cuda.synchronize()
    assert torch.equal(bits(q), bits(qr)) and torch.equal(bits(kc), bits(kr)) and torch.equal(bits(vc), bits(vr))
    for b, p in enumerate(POS):
        keep = torch.ones(Smax, dtype=torch.bool)
        keep[p:p + T] = False
        assert torch.equal(bits(kc[b][:, keep]), bits(kc0[b][:, keep])) and torch.equal(bits(vc[b][:, keep]), bits(vc0[b][:, keep]))
    assert not torch.equal(bits(kc), bits(kc0))


def test_rotary_at_tree_offsets(dev):
    """The slot is p + s, the angle that of p + off[s]: against the oracle's rotary at those positions."""
    from magma_amd import ops
    from oracle.model import apply_rotary
    rot, Smax, T = 64, 256, 40
    kc0, vc0, qkv, sin_t, cos_t = rotary_operands(dev, T, rot, Smax)
    g = torch.Generator().manual_seed(5)
    off = torch.stack([torch.minimum(torch.randint(0, 7, (T,), generator=g), torch.arange(T)) for _ in range(B)]).to(torch.int32)
    kc, vc = kc0.clone(), vc0.clone()
    q = torch.empty(B, H, T, 256, dtype=BF16, device=dev)
    ops.rotary_split_at(qkv, B, T, H, rot, sin_t, cos_t, q, kc, vc, torch.tensor(POS, dtype=torch.int32, device=dev), off.to(dev))
    x = qkv.view(B, T, 3, H, 256).float().cpu()
    for b, p in enumerate(POS):
        pt = p + off[b].to(torch.int64)
        k_new = apply_rotary(x[b:b + 1, :, 1], pt, rot)[0].transpose(0, 1)
        q_new = apply_rotary(x[b:b + 1, :, 0], pt, rot)[0].transpose(0, 1)
        assert rel(kc[b, :, p:p + T], k_new) <= 3e-3 and rel(q[b], q_new) <= 3e-3, f"row {b}"
        assert torch.equal(vc[b, :, p:p + T].float().cpu(), x[b, :, 2].transpose(0, 1)), f"appended v, row {b}"
        keep = torch.ones(Smax, dtype=torch.bool)
        keep[p:p + T] = False
        assert torch.equal(kc[b][:, keep], kc0[b][:, keep]) and torch.equal(vc[b][:, keep], vc0[b][:, keep]), f"row {b}: other slots"
    with pytest.raises(ValueError):
        ops.rotary_split_at(qkv, B, T, H, rot, sin_t, cos_t, q, kc, vc, torch.tensor(POS, dtype=torch.int32, device=dev),
                            off[:, :3].contiguous().to(dev))


# ------------------------------------------------------------------------------------------------------- log-probabilities
@pytest.mark.parametrize("V", [1056, 50258])
def test_token_logprobs_rows_gives_the_bits_of_token_logprobs(dev, V):
    from magma_amd import ops
    R, N = 5, 23
    ld = (V + 7) // 8 * 8 + 8
    logits = (rnd(R, ld, dev=dev, seed=31) * 4)[:, :V]
    g = torch.Generator().manual_seed(7)
    row_of = torch.randint(0, R, (N,), generator=g).to(torch.int32)
    token = torch.randint(0, V, (N,), generator=g).to(torch.int32)
    token[3], token[8], token[9] = V, -1, V - 1
    lp = torch.full((N,), float("nan"), dtype=torch.float32, device=dev)
    ops.token_logprobs_rows(logits, row_of.to(dev), token.to(dev), lp)
    ref = torch.full((N, 1), float("nan"), dtype=torch.float32, device=dev)
    ops.token_logprobs(logits[row_of.to(dev).to(torch.int64)].contiguous(), token.to(torch.int64).to(dev), ref)
    torch.cuda.synchronize()
    assert torch.equal(lp.view(torch.int32), ref[:, 0].view(torch.int32))
    assert float(lp[3]) == -math.inf and float(lp[8]) == -math.inf and math.isfinite(float(lp[9]))
    host = torch.log_softmax(logits.double().cpu(), -1)[row_of.to(torch.int64), token.clamp(0, V - 1).to(torch.int64)]
    ok = (token >= 0) & (token < V)
    assert float((lp.cpu().double() - host)[ok].abs().max()) <= 1e-4
    # a row outside the logits gives -inf and reads nothing
    row_of[0] = R
    ops.token_logprobs_rows(logits, row_of.to(dev), token.to(dev), lp)
    assert float(lp[0]) == -math.inf
