"""Ranking choices (DESIGN.md "Ranking choices"), the host side: TokenTrie.rows' preorder table, the tree forward stated in pure
torch on a tiny HF GPT-J -- ONE pass over [prompt ; nodes] under the mask built from ``sub`` at positions p + off -- against the
host statement of rank() (one forward per candidate), and rank()'s argument checks.  No GPU: the kernels and the engine are
tested against the same statements in tests/test_rank_kernels_gpu.py and tests/test_rank_gpu.py."""
import random
from types import SimpleNamespace

import pytest
import torch

from magma_amd.sampling import Ranking, TokenTrie, pad_trie_rows, rank, rank_groups
from test_beam_search_cpu import EOS, V, _tiny_gptj

CHAIN = [[4, 9, 2, 30, 11]]
STAR = [[t] for t in (3, 17, 5, 40, 8)]
MIXED = [[5, 6, 7], [5, 6], [5, 8, 1], [9], [5, 6, 7], [3, 1], [5, 8, 2], [9, 9, 9, 9]]          # a duplicate, prefixes of others


def _random_seqs(seed, n, vocab=12, longest=5):
    rng = random.Random(seed)
    return [[rng.randrange(vocab) for _ in range(rng.randint(1, longest))] for _ in range(n)]


def _walk(rows, leaf):
    """The rows from ``leaf`` up to a child of the root."""
    out, i = [], int(leaf)
    while i >= 0:
        out.append(i)
        i = int(rows.parent[i])
    return out


@pytest.mark.parametrize("seqs", [CHAIN, STAR, MIXED, _random_seqs(1, 40), _random_seqs(2, 200, vocab=5)],
                         ids=["chain", "star", "mixed", "random40", "random200"])
def test_rows_preorder_invariants(seqs):
    trie = TokenTrie(seqs)
    r = trie.rows()
    N = r.token.numel()
    assert N == trie.n_nodes - 1 and all(t.dtype == torch.int32 for t in r) and r.leaf_of.numel() == len(seqs)
    for i in range(N):
        pa = int(r.parent[i])
        assert -1 <= pa < i and int(r.off[i]) == (0 if pa < 0 else int(r.off[pa]) + 1) and i < int(r.sub[i]) <= N
    for c, q in enumerate(seqs):
        path = _walk(r, r.leaf_of[c])
        assert [int(r.token[i]) for i in reversed(path)] == list(q) and int(r.terminal[r.leaf_of[c]]) == 1
        assert [int(r.off[i]) for i in reversed(path)] == list(range(len(q)))
        i = int(r.leaf_of[c])
        for j in range(N):            # two compares say "j is i or an ancestor of i"
            assert (j <= i < int(r.sub[j])) == (j in path), (c, i, j)
    assert int(r.terminal.sum()) == len({tuple(q) for q in seqs})


def test_rows_of_a_chain_and_of_a_star():
    r = TokenTrie(CHAIN).rows()
    assert r.sub.tolist() == [5] * 5 and r.parent.tolist() == [-1, 0, 1, 2, 3] and r.off.tolist() == [0, 1, 2, 3, 4]
    r = TokenTrie(STAR).rows()
    assert r.sub.tolist() == [1, 2, 3, 4, 5] and r.parent.tolist() == [-1] * 5 and r.off.tolist() == [0] * 5
    assert r.token.tolist() == sorted(t[0] for t in STAR) and [int(r.token[i]) for i in r.leaf_of] == [t[0] for t in STAR]


def test_rows_padded_per_row_and_in_groups():
    a, b = TokenTrie(MIXED).rows(), TokenTrie(STAR).rows()
    token, off, sub = pad_trie_rows([a, None, b])
    T = a.token.numel()
    assert token.shape == off.shape == sub.shape == (3, T) and T > b.token.numel()
    assert torch.equal(sub[0], a.sub) and torch.equal(token[0], a.token) and torch.equal(off[0], a.off)
    n = b.token.numel()
    assert torch.equal(sub[2, :n], b.sub) and sub[2, n:].tolist() == list(range(n + 1, T + 1)) and not off[2, n:].any()
    assert sub[1].tolist() == list(range(1, T + 1)) and not off[1].any() and not token[1].any()
    # groups: whole sequences, every listed position once, each group within the budget, the first group's rows as in the whole trie
    trie = TokenTrie(MIXED)
    for budget in (4, 5, 7, 100):
        groups = rank_groups(trie, budget)
        assert sorted(c for g in groups for c in g) == list(range(len(MIXED)))
        for g in groups:
            rows = trie.rows(g)
            assert rows.token.numel() <= budget
            for c, leaf in zip(g, rows.leaf_of):
                assert [int(rows.token[i]) for i in reversed(_walk(rows, leaf))] == MIXED[c]
        first = trie.rows(groups[0])
        n = first.token.numel()
        assert torch.equal(first.token, a.token[:n]) and torch.equal(first.parent, a.parent[:n])
        assert [int(a.leaf_of[c]) for c in groups[0]] == first.leaf_of.tolist()
    assert len(rank_groups(trie, 100)) == 1 and len(rank_groups(trie, 4)) > 1
    with pytest.raises(ValueError):
        rank_groups(trie, 3)            # [9, 9, 9, 9] alone needs four nodes


# ------------------------------------------------------------------------------- the tree forward, stated in torch
@pytest.fixture(scope="module")
def tiny():
    from test_logits_processors_cpu import _HostMagma
    lm = _tiny_gptj(seed=4, eos_bias=1.5)
    emb = torch.randn(2, 6, 32, generator=torch.Generator().manual_seed(5))
    return _HostMagma(lm), emb


def _tree_terms(lm, prompt, trie, eos):
    """One pass over [prompt ; nodes]: node i at position p + off[i] under the additive mask "key j of the chunk iff
    j <= i < sub[j]".  Returns per listed sequence the list of its terms, root first, the eos term last."""
    r = trie.rows()
    p, N = prompt.shape[1], r.token.numel()
    x = torch.cat([prompt, lm.transformer.wte(r.token.to(torch.int64))[None]], 1)
    mask = torch.full((p + N, p + N), float("-inf")).triu(1)
    i, j = torch.arange(N)[:, None], torch.arange(N)[None, :]
    mask[p:, p:] = torch.where((j <= i) & (i < r.sub.to(torch.int64)[None, :]), 0.0, float("-inf"))
    pos = torch.cat([torch.arange(p), p + r.off.to(torch.int64)])[None]
    with torch.no_grad():
        ls = torch.log_softmax(lm(inputs_embeds=x, attention_mask=mask[None, None], position_ids=pos).logits[0].double(), -1)
    out = []
    for c, q in enumerate(trie.sequences):
        path = list(reversed(_walk(r, r.leaf_of[c])))
        src = [p - 1] + [p + n for n in path]               # the row that predicts each token (and the eos)
        terms = [float(ls[src[k], q[k]]) for k in range(len(q))]
        if eos:
            terms.append(float(ls[src[len(q)], EOS]))
        out.append(terms)
    return out


@pytest.mark.parametrize("eos", [True, False])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0])
def test_tree_forward_in_torch_equals_the_host_statement(tiny, eos, length_penalty):
    model, emb = tiny
    lens = torch.tensor([6, 4])
    tries = [TokenTrie(MIXED), TokenTrie([[2, 2, 3], [2], [40, 1]])]
    got, terms = rank(model, emb, tries, lengths=lens, eos=eos, length_penalty=length_penalty, return_terms=True)
    assert isinstance(got, Ranking) and got.logprobs.shape == (2, len(MIXED)) and got.index.dtype == torch.int64
    assert got.logprobs.dtype == got.scores.dtype == torch.float32 and got.count.dtype == torch.int64
    for b, trie in enumerate(tries):
        ref = _tree_terms(model.lm.inner, emb[b:b + 1, : int(lens[b])], trie, eos)
        n = len(trie.sequences)
        assert got.count[b, :n].tolist() == [len(q) + int(eos) for q in trie.sequences] and not got.count[b, n:].any()
        assert bool(torch.isinf(got.logprobs[b, n:]).all()) and bool(torch.isinf(got.scores[b, n:]).all())
        for c, t in enumerate(ref):
            # fp32 rounding of the two forwards: a log-probability of a few units carries ~1e-6
            assert torch.allclose(terms[b, c, : len(t)].double(), torch.tensor(t, dtype=torch.float64), rtol=0, atol=2e-5), (b, c)
            assert not terms[b, c, len(t):].any()
            assert abs(float(got.logprobs[b, c]) - sum(t)) <= 2e-5 * len(t)
            assert abs(float(got.scores[b, c]) - sum(t) / len(t) ** length_penalty) <= 2e-5 * len(t)
        best = max(range(n), key=lambda c: (float(got.scores[b, c]), -c))
        assert int(got.index[b]) == best
    # a duplicate gets its score twice, and the tie goes to the lower position
    assert float(got.logprobs[0, 0]) == float(got.logprobs[0, 4]) and int(got.index[0]) != 4


def test_index_is_the_argmax_of_the_sums(tiny):
    """rank's index is the arg-max of the host statement's sums, and a choice's sum does not depend on the other choices."""
    model, emb = tiny
    seqs = _random_seqs(3, 12, vocab=V - 2, longest=3)
    got = rank(model, emb, seqs, eos=True)
    assert got.index.tolist() == [int(torch.argmax(got.logprobs[b])) for b in range(2)]
    one = rank(model, emb[:1], [seqs[int(got.index[0])], seqs[0]])
    assert abs(float(one.logprobs[0, 0]) - float(got.logprobs[0, int(got.index[0])])) <= 1e-5


def test_argument_checks(tiny):
    model, emb = tiny
    for bad in (dict(eos=1), dict(eos=[EOS]), dict(length_penalty=float("nan")), dict(length_penalty="1"), dict(max_nodes=0)):
        with pytest.raises(ValueError):
            rank(model, emb, STAR, **bad)
    for choices in (None, [], [[]], [[-1]], [[V]], [STAR]):                        # one per-row entry for two rows
        with pytest.raises(ValueError):
            rank(model, emb, choices)
    with pytest.raises(ValueError):
        rank(model, emb, STAR, lengths=[6, 7])
    with pytest.raises(ValueError):
        rank(model, emb, STAR, lengths=[6])
    # positions: the tiny model has 64; a prompt of 6 leaves room for 58 tokens
    assert model.lm.config.max_position_embeddings == 64
    ok = [[1] * 58]
    rank(model, emb[:1], ok, eos=False)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        rank(model, emb[:1], [[1] * 59], eos=False)

    class _NoForward(SimpleNamespace):          # the check runs before the model is touched
        pass
    dead = _NoForward(eos_token=EOS, tokenizer=None, lm=SimpleNamespace(config=SimpleNamespace(vocab_size=V, max_position_embeddings=8)))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        rank(dead, emb, [[1, 2, 3]])
