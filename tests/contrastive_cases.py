"""Seeded inputs for the contrastive-search kernels (DESIGN.md "Contrastive search") and the error bound their tests share.

Both sides of every comparison start from the same bf16 vectors.  A length-d fp32 dot product and two fp32 sums of squares give
|dcos| <= 2 (d + 8) 2^-24 -- the worst-case summation bound in any order, the MFMA's included --, an fp32 softmax against fp64
|dp| <= 2^-16.  A selection is DECIDED when the reference's gap between the best and the second-best score exceeds
2 (alpha cos_bound(d) + (1 - alpha) 2^-16): then no arithmetic within the bounds selects another candidate.  The tests assert
decidedness of every case they compare; they never skip an undecided one."""
import math

import torch

BF16 = torch.bfloat16
CHUNK = 32                      # ops.CONTRASTIVE_CHUNK: context positions per workgroup of the similarity kernel
TMAX = 3 * CHUNK                # the store of the kernel cases: three chunks
P_BOUND = 2.0 ** -16
# context lengths: one position, either side of a chunk edge, into the third chunk, and the last length that leaves room to append
LENGTHS = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, TMAX - 1)
ADVERSARIAL = ("equal", "scaled", "zero_row", "last_valid", "past_len")


def cos_bound(d: int) -> float:
    return 2.0 * (d + 8) * 2.0 ** -24


def gap_bound(alpha: float, d: int) -> float:
    return 2.0 * (alpha * cos_bound(d) + (1.0 - alpha) * P_BOUND)


def ragged_lengths(T: int, B: int = 3):
    """B context lengths, the first one T, the others on other sides of the chunk edges."""
    return [T, max(1, T // 2), max(1, T - CHUNK)][:B] + [max(1, T - 3)] * max(0, B - 3)


def sim_case(d: int, k: int, T: int, seed: int, alpha: float = 0.6, B: int = 3, adversarial: str = None):
    """_draw's case for the first of the seeds seed, seed + 7919, ... at which the REFERENCE's selection is decided with four times
    the margin (judged by the host statement alone, before any kernel sees the input): sixteen scores on a grid now and then land
    within 1e-4 of each other."""
    for attempt in range(8):
        case = _draw(d, k, T, seed + 7919 * attempt, alpha, B, adversarial)
        if float(reference(case)[3].min()) > 4 * gap_bound(alpha, d):
            return case
    raise AssertionError(f"no decided input for {(d, k, T, seed, adversarial)}")


def _draw(d, k, T, seed, alpha, B, adversarial):
    """One case of the similarity + selection kernels: ``ctx`` (B, TMAX, d) bf16 with ``ctx_len`` = ragged_lengths(T) valid rows
    per sample (the rows beyond hold random values too: they must be masked, not merely zero), ``hidden`` (B, k, d) bf16, ``p``
    (B, k) fp32.  Candidate j of a sample leans on one valid context row with a weight of its own -- a permutation of a grid over
    [0.1, 0.9] -- so the penalties, and with them the selected index, differ from candidate to candidate; the probabilities are a
    permutation of a gapped grid.

    ``adversarial`` changes sample 0: "equal" -- candidate 0 IS a context row (cosine 1); "scaled" -- candidate 0 is a context row
    times 3 (cosine still 1); "zero_row" -- a zero context row and a zero candidate (cosine 0 by definition, never NaN);
    "last_valid" -- the best position of candidate 0 is the last valid one; "past_len" -- the row ONE PAST ctx_len equals candidate 0
    and must be ignored."""
    g = torch.Generator().manual_seed(seed)
    lens = ragged_lengths(T, B)
    ctx = torch.randn(B, TMAX, d, generator=g)
    hidden = torch.zeros(B, k, d)
    grid = torch.linspace(0.1, 0.9, max(k, 2))[:k]
    for b in range(B):
        w = grid[torch.randperm(k, generator=g)]
        at = torch.randint(0, lens[b], (k,), generator=g)
        noise = torch.randn(k, d, generator=g)
        hidden[b] = w[:, None] * ctx[b, at] + (1 - w * w).sqrt()[:, None] * noise
    pg = (torch.arange(k, dtype=torch.float32) + 1.0) * (0.8 / (k * (k + 1) / 2))       # gapped, sums to 0.8
    p = torch.stack([pg[torch.randperm(k, generator=g)] for _ in range(B)])
    ctx, hidden = ctx.to(BF16), hidden.to(BF16)
    n0 = lens[0]
    if adversarial == "equal":
        hidden[0, 0] = ctx[0, n0 // 2]
    elif adversarial == "scaled":
        hidden[0, 0] = (ctx[0, n0 // 2].float() * 3.0).to(BF16)
    elif adversarial == "zero_row":
        ctx[0, n0 // 2] = 0
        hidden[0, k - 1] = 0
    elif adversarial == "last_valid":
        hidden[0, 0] = ctx[0, n0 - 1]
    elif adversarial == "past_len":
        assert n0 < TMAX
        ctx[0, n0] = hidden[0, 0]
    elif adversarial is not None:
        raise ValueError(adversarial)
    return dict(ctx=ctx, ctx_len=torch.tensor(lens, dtype=torch.int32), hidden=hidden, p=p, alpha=alpha, d=d, k=k)


def reference(case):
    """(selected, score, penalty, gap) of a case by the host statement; gap (B,) = best less second-best score (inf at k = 1)."""
    from magma_amd.sampling import contrastive_rank
    sel, score, pen = contrastive_rank(case["ctx"], case["ctx_len"], case["hidden"], case["p"], case["alpha"])
    k = case["k"]
    top2 = torch.topk(score, min(2, k), dim=-1).values
    gap = top2[:, 0] - top2[:, 1] if k > 1 else torch.full((score.shape[0],), math.inf, dtype=torch.float64)
    return sel, score, pen, gap


def kernel_cases():
    """(d, k, T, adversarial) of every similarity-kernel case: the grid of hidden sizes, candidate counts and context lengths,
    then the adversarial inputs at a length inside the second chunk."""
    cases = [(d, k, T, None) for d in (256, 512, 4096) for k in (1, 2, 5, 16) for T in LENGTHS]
    cases += [(512, 5, CHUNK + 9, a) for a in ADVERSARIAL] + [(4096, 16, 2 * CHUNK + 1, a) for a in ADVERSARIAL]
    return cases


def case_seed(d, k, T, adversarial):
    return d * 31 + k * 7 + T + (0 if adversarial is None else 1000 + ADVERSARIAL.index(adversarial))
