"""Constrained decoding on the host (DESIGN.md "Constrained decoding"): TokenTrie's construction, limits and table; the host
rule (magma_amd.sampling.constrain_logits) against the installed transformers' PrefixConstrainedLogitsProcessor as values; the
argument checks of generate(); the host branch of generate(constraint=...) and choose() on the tiny random GPT-J of
tests/test_beam_search_cpu.py.  No GPU: the device kernel is tested against the same host rule in tests/test_constrained_gpu.py."""
from types import SimpleNamespace

import pytest
import torch

from magma_amd.sampling import (TokenTrie, check_constraint_args, check_processor_args, choose, constrain_logits, generate,
                                process_logits, trie_forest)
from test_beam_search_cpu import EOS, V, _tiny_gptj

SEQS = [[5, 6, 9], [5, 6], [5, 11], [12], [0, V - 1, 3], [5, 6, 9]]        # a prefix of another, a duplicate, ids 0 and V - 1


# ------------------------------------------------------------------------------------------------------------- the trie
def test_trie_construction_index_and_table_round_trip():
    trie = TokenTrie(SEQS)
    assert trie.sequences == tuple(tuple(q) for q in SEQS)
    assert [trie.index(q) for q in SEQS] == [0, 1, 2, 3, 4, 0]              # a duplicate: the first position
    assert trie.index([5]) == -1 and trie.index([5, 6, 9, 9]) == -1 and trie.index([]) == -1
    assert trie.index(torch.tensor([5, 11])) == 2
    assert trie.n_nodes == 1 + 3 + 3 + 2 and trie.n_edges == trie.n_nodes - 1      # duplicates collapsed
    assert trie.min_len() == 1 and trie.max_len() == 3 and trie.tokens() == {0, 3, 5, 6, 9, 11, 12, V - 1}
    table = trie.flat()
    n, e = trie.n_nodes, trie.n_edges
    assert table.dtype == torch.int32 and table.numel() == 3 + 4 * n + 2 * e and table[:2].tolist() == [n, e]
    first = table[2: 3 + n].tolist()
    etok = table[3 + 4 * n: 3 + 4 * n + e].tolist()
    assert first[0] == 0 and first[-1] == e and first == sorted(first)
    for i in range(n):                                                       # ascending and distinct within a node
        toks = etok[first[i]: first[i + 1]]
        assert toks == sorted(set(toks))
    terminal = table[3 + n: 3 + 2 * n].tolist()
    assert all(terminal[i] for i in range(n) if first[i] == first[i + 1])   # a leaf is terminal
    assert sorted(TokenTrie.from_flat(table)) == sorted(set(tuple(q) for q in SEQS))
    # the walk: an inner node, a terminal inner node, a leaf, off the trie
    assert trie.allowed([], [EOS]) == [0, 5, 12]
    assert trie.allowed([5], [EOS, 2]) == [6, 11]
    assert trie.allowed([5, 6], [EOS, 2]) == [9, EOS, 2]
    assert trie.allowed([5, 6, 9], [EOS]) == [EOS] and trie.allowed([5, 7], [EOS]) == [EOS]
    assert trie.allowed([12, EOS, EOS], [EOS]) == [EOS]
    with pytest.raises(AttributeError):
        trie.sequences = ()


def test_trie_strings_and_validation():
    enc = lambda s: [ord(c) - 90 for c in s]  # noqa: E731
    trie = TokenTrie(["ab", [9, 9], "b"], encode=enc)
    assert trie.index([7, 8]) == 0 and trie.index([8]) == 2
    for bad in ([], [[]], [[1, -1]], [[1.0]], [[True]], ["ab"], "ab", [[1] * 65], None, [3]):
        with pytest.raises(ValueError):
            TokenTrie(bad)
    TokenTrie([[1] * 64])
    with pytest.raises(ValueError):
        TokenTrie([[i] for i in range(65537)])
    assert TokenTrie([[i] for i in range(65536)]).n_nodes == 65537
    # 2^20 nodes at most: 16 500 sequences of 64 distinct-from-the-start ids need 1 056 001
    with pytest.raises(ValueError, match="nodes"):
        TokenTrie([[i] * 64 for i in range(16500)])


def test_forest_shifts_nodes_and_edges():
    a, b = TokenTrie([[1, 2], [3]]), TokenTrie([[4], [4, 5], [6]])
    table, roots = trie_forest([a, b, a])
    assert roots.tolist() == [0, a.n_nodes, 0]
    n, e = a.n_nodes + b.n_nodes, a.n_edges + b.n_edges
    assert table[:2].tolist() == [n, e] and table.numel() == 3 + 4 * n + 2 * e
    parent = table[3 + 2 * n: 3 + 3 * n].tolist()
    assert [i for i, p in enumerate(parent) if p < 0] == [0, a.n_nodes]
    echild = table[3 + 4 * n + e:].tolist()
    assert sorted(echild) == [i for i in range(n) if i not in (0, a.n_nodes)]


def test_refused_combinations():
    trie = TokenTrie(SEQS)

    class _NoModel:            # the checks run before generate() touches the model
        eos_token = EOS
        training = False
        tokenizer = None
        lm = SimpleNamespace(config=SimpleNamespace(vocab_size=V))

    emb = torch.zeros(2, 2, 8)
    bad = [dict(no_repeat_ngram_size=2), dict(min_new_tokens=2), dict(suppress_tokens=[9]), dict(suppress_tokens=[EOS]),
           dict(eos_token=[EOS, 2], suppress_tokens=[2])]
    for kw in bad:
        with pytest.raises(ValueError):
            generate(_NoModel(), emb, max_steps=2, constraint=trie, **kw)
    for c in (TokenTrie([[V]]), [[1, V]], [trie], [trie, trie, trie], [], "ab", ["ab"], 7, [[1], [[2]]]):
        with pytest.raises(ValueError):
            generate(_NoModel(), emb, max_steps=2, constraint=c)
    for kw in (dict(num_beams=2), dict(return_scores=True)):
        with pytest.raises(NotImplementedError):
            generate(_NoModel(), emb, max_steps=2, constraint=trie, **kw)
    with pytest.raises(TypeError):          # keyword-only
        generate(_NoModel(), emb, 2, 0.0, 0, 0.9, EOS, False, True, None, None, None, 1, 1.0, False, 1, False, None, False, trie)
    # what is allowed: min_new_tokens up to the shortest sequence, a penalty, suppress ids beside the trie
    proc = check_processor_args(1.3, 0, 1, [4], V)
    tries = check_constraint_args(trie, 3, None, V, (EOS,), proc)
    assert len(tries) == 3 and all(t is trie for t in tries)
    shared = check_constraint_args(SEQS, 2, None, V)
    assert shared[0] is shared[1] and shared[0].sequences == trie.sequences
    rows = check_constraint_args([SEQS, [[1], [2]]], 2, None, V)
    assert rows[0].sequences == trie.sequences and rows[1].sequences == ((1,), (2,))
    assert check_constraint_args(None, 2) is None


# ----------------------------------------------------------------------------------------- the host rule and transformers
def _hf(tries, eos_ids):
    from transformers import PrefixConstrainedLogitsProcessor
    return PrefixConstrainedLogitsProcessor(lambda b, ids: tries[b].allowed(ids.tolist(), eos_ids), 1)


HISTORIES = {"root": [], "inner": [5], "terminal inner": [5, 6], "leaf": [5, 6, 9], "off": [5, 7, 6], "after eos": [12, EOS, EOS],
             "leaf with 0": [0, V - 1, 3], "eos at once": [EOS]}


@pytest.mark.parametrize("eos_ids", [(EOS,), (EOS, 2, 40)])
@pytest.mark.parametrize("per_row", [False, True])
def test_host_rule_equals_prefix_constrained_processor(per_row, eos_ids):
    pytest.importorskip("transformers")
    g = torch.Generator().manual_seed(len(eos_ids) + per_row)
    other = TokenTrie([[5, 7], [5, 7, 6, 1], [EOS, 3], [30]])
    for name, h in HISTORIES.items():
        R = 3
        tries = [TokenTrie(SEQS), other, TokenTrie(SEQS)] if per_row else [TokenTrie(SEQS)] * R
        x = torch.randn(R, V, generator=g) * 3
        x[0, 5], x[1, 6] = float("-inf"), 0.0
        hist = torch.tensor([h] * R, dtype=torch.int64).view(R, len(h))
        ref = _hf(tries, eos_ids)(hist, x.clone())
        got = constrain_logits(x, hist, len(h), tries if per_row else tries[0], eos_ids)
        assert torch.equal(got, ref), (name, (got != ref).nonzero())
        wide = torch.cat([hist, torch.full((R, 3), 5)], dim=1)                # only the first `step` columns count
        assert torch.equal(constrain_logits(x, wide, len(h), tries, eos_ids), ref), name
        assert bool((got > float("-inf")).any(1).all()) and not torch.equal(got, x), name


def test_host_rule_chained_behind_the_penalty():
    pytest.importorskip("transformers")
    from transformers import LogitsProcessorList, RepetitionPenaltyLogitsProcessor
    trie = TokenTrie(SEQS)
    g = torch.Generator().manual_seed(3)
    for h in ([5], [5, 6], [5, 6, 9], [12, EOS]):
        x = torch.randn(2, V, generator=g) * 3
        hist = torch.tensor([h, h], dtype=torch.int64)
        ref = LogitsProcessorList([RepetitionPenaltyLogitsProcessor(penalty=1.7), _hf([trie, trie], (EOS,))])(hist, x.clone())
        got = constrain_logits(process_logits(x, hist, len(h), repetition_penalty=1.7), hist, len(h), trie, (EOS,))
        assert torch.equal(got, ref), h


# ------------------------------------------------------------------------------------------ generate()'s host branch
N = 8


@pytest.fixture(scope="module")
def tiny():
    from test_logits_processors_cpu import _HostMagma
    model = _tiny_gptj(seed=4, eos_bias=1.5)
    emb = torch.randn(3, 5, 32, generator=torch.Generator().manual_seed(11))
    return _HostMagma(model), emb


def _listed(row, trie):
    """Is the id row a listed sequence followed by eos padding?"""
    row = row.tolist()
    n = row.index(EOS) if EOS in row else len(row)
    return trie.index(row[:n]) >= 0 and all(t == EOS for t in row[n:])


def _choices(plain):
    """Sequences none of which starts with a token the plain run starts with."""
    first = {int(t) for t in plain[:, 0]}
    free = [t for t in range(V) if t not in first and t != EOS]
    return [[free[0], free[1], free[2]], [free[0], free[1]], [free[3]], [free[4], free[0]]]


def test_generate_host_branch_stays_inside_the_trie(tiny):
    model, emb = tiny
    S = emb.shape[1]
    plain = generate(model, emb, max_steps=N, temperature=0.0, eos_token=EOS, decode=False, stop_on_eos=False)[:, S:]
    trie = TokenTrie(_choices(plain))
    assert not any(_listed(r, trie) for r in plain)
    got = generate(model, emb, max_steps=N, temperature=0.0, eos_token=EOS, decode=False, stop_on_eos=False, constraint=trie)[:, S:]
    assert got.shape == (3, N) and all(_listed(r, trie) for r in got), got
    # the same through the list form, per row, and sampled
    rows = [trie.sequences, [list(trie.sequences[2])], trie]
    per = generate(model, emb, max_steps=N, temperature=0.0, eos_token=EOS, decode=False, stop_on_eos=False, constraint=rows)[:, S:]
    assert torch.equal(per[0], got[0]) and torch.equal(per[2], got[2])
    assert per[1].tolist() == list(trie.sequences[2]) + [EOS] * (N - 1)
    torch.manual_seed(0)
    smp = generate(model, emb, max_steps=N, temperature=1.5, top_k=0, top_p=0.0, eos_token=EOS, decode=False, stop_on_eos=False,
                   constraint=list(trie.sequences))[:, S:]
    assert all(_listed(r, trie) for r in smp), smp
    # the host loop stated once more: raw logits, the rule, argmax
    lm = model.lm.inner
    with torch.no_grad():
        o = lm(inputs_embeds=emb, use_cache=True)
        hist = torch.zeros(3, N, dtype=torch.int64)
        for t in range(N):
            x = constrain_logits(o.logits[:, -1].float(), hist, t, trie, (EOS,))
            hist[:, t] = x.argmax(-1)
            o = lm(input_ids=hist[:, t:t + 1], past_key_values=o.past_key_values, use_cache=True)
    assert torch.equal(got, hist)


def test_choose_maps_rows_back_to_their_choices(tiny):
    model, emb = tiny
    S = emb.shape[1]
    plain = generate(model, emb, max_steps=N, temperature=0.0, eos_token=EOS, decode=False, stop_on_eos=False)[:, S:]
    seqs = _choices(plain)
    trie = TokenTrie(seqs)
    got = generate(model, emb, max_steps=N, temperature=0.0, eos_token=EOS, decode=False, stop_on_eos=False, constraint=trie)[:, S:]
    want = [trie.index(r.tolist()[: r.tolist().index(EOS)]) for r in got]
    index, lp = choose(model, emb, seqs, eos_token=EOS)
    assert index.dtype == torch.int64 and index.tolist() == want and min(want) >= 0
    assert lp.count.tolist() == [len(seqs[i]) + 1 for i in want]
    assert bool((lp.logprobs <= 0).all()) and lp.tokens.shape[1] <= trie.max_len() + 1
    per_row, _ = choose(model, emb, [seqs, seqs[2:], seqs[::-1]], eos_token=EOS)
    assert per_row[0] == index[0] and per_row[2] == len(seqs) - 1 - index[2] and 0 <= per_row[1] < 2
    with pytest.raises(ValueError):
        choose(model, emb, seqs, max_steps=3)
