"""Fixtures that the diverse-beam-search tests share (tests/test_group_beam_cpu.py, tests/test_group_beam_gpu.py): scripted
per-step logits in the style of tests/test_beam_search_gpu.py's, a toy model whose logits depend on a row's own history alone,
and the host statement run on either with its parents and its record kept."""
import torch


def gapped_logits(R, V, seed, gap=1e-3):
    """Row logits that are a random permutation of an evenly spaced grid: no ties, and any two scores of a row differ by
    >= gap, so the comparison with a float64 statement is exact whatever the rounding of the logsumexp."""
    g = torch.Generator().manual_seed(seed)
    base = torch.arange(V, dtype=torch.float64) * gap * 4
    rows = [base[torch.randperm(V, generator=g)] - 0.5 * V * gap * 4 + torch.randn(1, generator=g, dtype=torch.float64)
            for _ in range(R)]
    return torch.stack(rows).float()


def scripted(k, lp, es, eos_mode, B=3, V=64, n=10, eos=5, same_first=False, salt=0):
    """Logits per step over B*k rows.  "random": eos boosted by a random amount per step (it lands among the first candidates
    and outside them, some hypotheses finish early, the others at max_steps).  "heavy": from step 1 on eos tops every row, so
    the slots fill within a few steps and generation stops before max_steps.  Every row and step has its own spread, so no two
    candidate sums tie across beams.  ``same_first``: at step 0 all rows of a sample hold the same logits (one prompt)."""
    R = B * k
    g = torch.Generator().manual_seed(100 * k + int(lp * 10) + len(str(es)) + 7919 * salt)
    scale = 200 + 200 * torch.rand(n, R, 1, generator=g, dtype=torch.float64)
    table = [(gapped_logits(R, V, seed=1000 * (salt + 1) + t).double() * scale[t]).float() for t in range(n)]
    for t in range(n):
        if eos_mode == "random":
            table[t][:, eos] += float(torch.rand(1, generator=g)) * 10 - 3
        elif t >= 1:
            table[t][:, eos] = table[t].max(-1).values + 1.0 + 5 * torch.rand(R, generator=g)
    if same_first:
        table[0] = table[0].view(B, k, V)[:, :1].expand(B, k, V).reshape(R, V).contiguous()
    return table


def host_run(table, B, k, G, lam, n, eos, lp, es, n_ret=None, plain=False):
    """group_beam_search (``plain``: beam_search, G and lam unused) on scripted logits: (result, parents per step, record)."""
    from magma_amd.sampling import beam_search, group_beam_search
    parents, rec = [], []

    def step(rows, tokens):
        if rows is not None:
            parents.append(rows.clone())
        return table[len(parents)]

    if plain:
        return beam_search(step, B, k, n, eos, lp, es, n_ret or k, record=rec), parents, rec
    return group_beam_search(step, B, k, G, lam, n, eos, lp, es, n_ret or k, record=rec), parents, rec


# The device forms log_softmax with its own reduction tree, so a candidate score differs from the host statement's by a few
# ulp -- 1e-6 at the scores' magnitude of 10, at most 1e-5 summed over 10 steps.  A fixture is used only if every pair of
# values that a decision of the HOST run compares (beam_margin) is ten times further apart than that.
DECISION_MARGIN = 1e-4


def scripted_run(k, G, lam, lp, es, eos_mode, B=3, V=64, n=10, eos=5, same_first=False):
    """The first of the scripted fixtures (salt 0, 1, ...) whose host run keeps DECISION_MARGIN, chosen from the host
    statement's record alone: (table, result, parents, record)."""
    from magma_amd.sampling import beam_margin
    for salt in range(16):
        table = scripted(k, lp, es, eos_mode, B, V, n, eos, same_first, salt)
        result, parents, rec = host_run(table, B, k, G, lam, n, eos, lp, es)
        if beam_margin(rec) >= DECISION_MARGIN:
            return table, result, parents, rec
    raise AssertionError("no scripted fixture with a safe decision margin")


class Toy:
    """A model whose logits depend only on the step and the row's last token (a fixed random table) with eos boosted from
    ``eos_from`` on: rows of different groups with the same history get the same logits."""

    def __init__(self, V=40, n=8, eos=3, seed=0, eos_from=2, boost=2.0):
        g = torch.Generator().manual_seed(seed)
        self.V, self.n, self.eos = V, n, eos
        self.first = torch.randn(V, generator=g) * 2
        self.table = torch.randn(n, V, V, generator=g) * 2
        self.table[eos_from:, :, eos] += boost

    def stepper(self, rows_total):
        t = [0]

        def step(rows, tokens):
            if rows is None:
                return self.first[None, :].expand(rows_total, self.V).contiguous()
            t[0] += 1
            return self.table[t[0], tokens]

        return step
