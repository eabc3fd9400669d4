"""Diverse beam search (DESIGN.md "Diverse beam search"): the host statement magma_amd.sampling.group_beam_search against
beam_search -- one group is beam search; group 0 is beam search with k' beams at any penalty; at penalty 0 every group is --,
against the closed form of its first step, and the argument checks.  No GPU: the device kernel is tested against the same
host statement in tests/test_group_beam_gpu.py."""
import pytest
import torch

import group_beam_cases as GC
from magma_amd.sampling import beam_margin, beam_search, check_beam_args, check_group_args, generate, group_beam_search


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("lp", [1.0, 0.0, -0.5])
@pytest.mark.parametrize("es", [True, False, "never"])
def test_one_group_is_beam_search(k, lp, es):
    for mode in ("random", "heavy"):
        table = GC.scripted(k, lp, es, mode)
        (a_seq, a_sc, a_len), a_par, _ = GC.host_run(table, 3, k, 1, 0.0, 10, 5, lp, es, plain=True)
        (b_seq, b_sc, b_len), b_par, _ = GC.host_run(table, 3, k, 1, 0.0, 10, 5, lp, es)
        assert torch.equal(a_seq, b_seq) and torch.equal(a_sc, b_sc) and torch.equal(a_len, b_len)
        assert len(a_par) == len(b_par) and all(torch.equal(p, q) for p, q in zip(a_par, b_par))


def _toy_runs(lam, n_ret, B=2, k=4, G=2, **kw):
    toy = GC.Toy(**kw)
    ref = beam_search(toy.stepper(B * k // G), B, k // G, toy.n, toy.eos, 1.0, False, k // G)
    got = group_beam_search(toy.stepper(B * k), B, k, G, lam, toy.n, toy.eos, 1.0, False, n_ret)
    return ref, got


def test_group_zero_is_beam_search_with_its_beams():
    """Group 0 is never penalised and reads nothing of the other groups: n_ret = 1 is beam_search with k' = 2 beams."""
    (seq, sc, lens), (g_seq, g_sc, g_len) = _toy_runs(0.7, 1)
    n = g_seq.shape[1]
    assert torch.equal(g_len, lens[0::2]) and torch.equal(g_sc, sc[0::2])
    assert torch.equal(g_seq, seq[0::2, :n]) and bool((seq[0::2, n:] == 3).all())
    assert bool((lens < 8).any()), "the toy must finish a hypothesis before max_steps"


def test_zero_penalty_gives_equal_groups():
    """lambda = 0 with G = 2: both groups are that k' = 2 run, so the round-robin output is each hypothesis twice."""
    (seq, sc, lens), (g_seq, g_sc, g_len) = _toy_runs(0.0, 4)
    twice = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3])                 # per sample: h0 (group 0), h0 (group 1), h1, h1
    assert torch.equal(g_seq, seq[twice]) and torch.equal(g_sc, sc[twice]) and torch.equal(g_len, lens[twice])


@pytest.mark.parametrize("k,G", [(4, 2), (6, 3), (16, 16)])
def test_first_step_closed_form(k, G):
    """Identical rows and a penalty larger than the spread of the log-probabilities: after step 0 group g runs on the tokens
    of ranks [g k', (g + 1) k') of the distribution, and its top 2k' are the ranks [g k', g k' + 2k')."""
    B, V, kq = 2, 64, k // G
    g = torch.Generator().manual_seed(k)
    dist = torch.randn(B, V, generator=g) * 3
    eos = int(dist.sum(0).argmin())
    dist[:, eos] = dist.min() - 5.0                                # eos is the last rank of both samples: nothing finishes
    order = torch.sort(dist, dim=-1, descending=True)[1]
    rec, fed = [], []

    def step(rows, tokens):
        fed.append(tokens)
        return dist.repeat_interleave(k, dim=0) if rows is None else torch.randn(B * k, V, generator=g)

    group_beam_search(step, B, k, G, 1e4, 2, eos, record=rec)      # two steps: at the last one every candidate finishes
    assert [r["group"] for r in rec[:G]] == list(range(G)) and all(r["step"] == 0 for r in rec[:G])
    for r in rec[:G]:
        lo = r["group"] * kq
        assert torch.equal(r["top_tok"], order[:, lo: lo + 2 * kq])
        assert torch.equal(r["row_rank"], torch.arange(lo, lo + 2 * kq).expand(B, 2 * kq))
        assert bool((r["top_beam"] == 0).all()) and torch.equal(r["running"], torch.arange(kq).expand(B, kq))
    assert torch.equal(fed[1].view(B, k), order[:, :k])             # what step 1 is fed: the running tokens of step 0


def test_validation():
    assert check_beam_args(4, 2, "never", 2, 0.5) == "never" and check_group_args(4, 2, 0) == (2, 0.0)
    assert check_group_args(6, 3, 1.5, vocab=8) == (3, 1.5) and check_group_args(16, 16, 0.0, vocab=17) == (16, 0.0)
    for k, G, lam, vocab in [(4, 0, 0.0, None), (4, -1, 0.0, None), (4, 3, 0.0, None), (4, 8, 0.0, None), (4, 2.0, 0.0, None),
                             (4, True, 0.0, None), (4, 2, -0.1, None), (4, 2, float("inf"), None), (4, 2, float("nan"), None),
                             (4, 2, "1", None), (4, 1, 0.5, None), (4, 2, 0.5, 5), (16, 16, 0.0, 16)]:
        with pytest.raises(ValueError):
            check_beam_args(k, 1, False, G, lam, vocab)
    with pytest.raises(ValueError):                                # the statement itself checks V against the logits it gets
        group_beam_search(lambda rows, tokens: torch.zeros(4, 5), 1, 4, 2, 0.5, 3, 0)

    class _NoModel:            # the checks run before generate() touches the model
        eos_token = 7
        training = False

    emb = torch.zeros(1, 2, 8)
    for kw in [dict(num_beams=4, num_beam_groups=3), dict(num_beams=4, num_beam_groups=2, diversity_penalty=-1.0),
               dict(num_beams=4, diversity_penalty=0.5), dict(num_beams=1, num_beam_groups=2),
               dict(num_beams=4, num_beam_groups=2, num_return_sequences=5)]:
        with pytest.raises(ValueError):
            generate(_NoModel(), emb, max_steps=2, **kw)
    # what beam search refuses stays refused, in the same words, with groups set
    groups = dict(num_beam_groups=2, diversity_penalty=0.5)
    for kw in [dict(stop_sequences=[[1, 2]]), dict(eos_token=[7, 8]), dict(return_finish=True), dict(return_logprobs=True),
               dict(top_logprobs=2, return_logprobs=True), dict(constraint=[[1, 2]]),
               dict(guidance_scale=2.0, negative_embeddings=torch.zeros(1, 2, 8)), dict(return_past_key_values=True)]:
        said = []
        for more in ({}, groups):
            with pytest.raises(NotImplementedError) as e:
                generate(_NoModel(), emb, max_steps=2, num_beams=4, **kw, **more)
            said.append(str(e.value))
        assert said[0] == said[1]


def test_record_gives_a_margin():
    """record= holds beam_search's values per step and group, on the penalised scores: beam_margin reads it unchanged.  The
    fixture must finish a group's hypothesis before max_steps and penalise a candidate that still reaches a top list."""
    B, k, G, lam, n = 3, 4, 2, 0.5, 10
    table = GC.scripted(k, 1.0, False, "random")
    _, parents, rec = GC.host_run(table, B, k, G, lam, n, 5, 1.0, False)
    assert len(rec) == G * (len(parents) + 1) and [r["group"] for r in rec[:G]] == [0, 1]
    assert any(bool((r["finished"] & (r["step"] + 1 < n)).any()) for r in rec)
    assert any(bool((r["top_n"] > 0).any()) for r in rec if r["group"] > 0)
    assert all(bool((r["counts"] == 0).all()) for r in rec if r["group"] == 0)
    for r in rec:       # the recorded top list is the penalised one: unpenalised scores of a row less lam * n_t
        assert r["top"].shape == (B, k + 1) and bool((r["top"][:, :-1] >= r["top"][:, 1:]).all())
    m = beam_margin(rec)
    assert 0 < m < float("inf")
