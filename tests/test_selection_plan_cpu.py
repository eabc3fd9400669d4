"""SelectionPlan (magma_amd/selection.py): the one checked statement of a token step's selection modes.  No engine, no GPU: the
constructor only normalises and refuses, and the key of a captured step is a pure function of the plan.

The key contract: two steps share a captured graph exactly when everything that is a LAUNCH ARGUMENT of the step agrees --
values and counts, never the contents of a device table that is rewritten between replays."""
import itertools

import pytest
import torch

from magma_amd.engine import KVCache, LMEngine
from magma_amd.sampling import TokenTrie

V = 1056
SAMPLED = (0.7, 5, 0.9)
BEAM = (2, 1.0, False, 8)
GUIDE = (1.5, 0.05)


def plan(vocab=V, **kw):
    return LMEngine.selection_plan(vocab=vocab, **kw)


def procs(ids, **kw):
    return dict(dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=1, suppress_tokens=ids), **kw)


def tries(*seqs):
    return [TokenTrie([list(q) for q in seqs])] * 2


# (what the pair is, plan a, plan b, the keys are equal)
PAIRS = [
    ("same processor values, other suppress ids of equal count", plan(processors=procs([11, 12])), plan(processors=procs([13, 14])), True),
    ("another suppress-id count", plan(processors=procs([11, 12])), plan(processors=procs([11, 12, 13])), False),
    ("another processor value", plan(processors=procs([11, 12])), plan(processors=procs([11, 12], repetition_penalty=1.4)), False),
    ("same eos / stop counts and pad id, other stop tokens", plan(stop=dict(eos_ids=[0, 7], stop_seqs=[[21, 22]])),
     plan(stop=dict(eos_ids=[0, 9], stop_seqs=[[23, 24, 25]])), True),
    ("another pad id", plan(stop=dict(eos_ids=[0, 7])), plan(stop=dict(eos_ids=[3, 7])), False),
    ("another stop count", plan(stop=dict(eos_ids=[0, 7])), plan(stop=dict(eos_ids=[0, 7], stop_seqs=[[21]])), False),
    ("two different tries", plan(constraint=tries([31, 32], [33])), plan(constraint=tries([41], [42, 43, 44])), True),
    ("a trie against no trie", plan(constraint=tries([31, 32])), plan(), False),
    ("another n_top", plan(logprobs=0), plan(logprobs=3), False),
    ("n_top 0 against no log-probabilities", plan(logprobs=0), plan(), False),
    ("another guidance scale", plan(guidance=GUIDE), plan(guidance=(2.0, 0.05)), False),
    ("another guidance cut", plan(guidance=GUIDE), plan(guidance=(1.5, 0.0)), False),
    ("a beam plan against a sampled plan", plan(beam=BEAM), plan(sampling=SAMPLED), False),
    ("the reference's sampler against transformers'", plan(sampling=SAMPLED), plan(sampling=("warp",) + SAMPLED + (0.0,)), False),
    ("equal plans built twice", plan(sampling=SAMPLED, processors=procs([11]), logprobs=2),
     plan(sampling=SAMPLED, processors=procs([11]), logprobs=2), True),
]


@pytest.mark.parametrize("what,a,b,equal", PAIRS, ids=[p[0] for p in PAIRS])
def test_graph_key_contract(what, a, b, equal):
    for feed_back in (False, True):
        ka, kb = a.graph_key(feed_back), b.graph_key(feed_back)
        assert hash(ka) == hash(ka) and (ka == kb) is equal, what
        assert (len({ka: 0, kb: 1}) == 1) is equal, what           # as keys of st.graphs


def test_feed_back_is_part_of_the_key():
    for p in (plan(), plan(sampling=SAMPLED), plan(beam=BEAM), plan(processors=procs([11]), logprobs=1)):
        assert p.graph_key(True) != p.graph_key(False)
        assert p.graph_key(True) == p.graph_key(True) and p.graph_key(True).feed_back is True


def test_key_fields_name_what_the_cache_drops_graphs_by():
    k = plan(constraint=tries([31]), logprobs=3).graph_key(True)
    assert k.constrained and k.n_top == 3 and not k.beam
    k = plan(beam=BEAM).graph_key(True)
    assert k.beam and not k.constrained and k.n_top is None
    k = plan(sampling=SAMPLED).graph_key(False)
    assert not k.beam and not k.constrained and k.n_top is None


def test_without_selection_drops_every_mode():
    full = plan(sampling=SAMPLED, processors=procs([11]), stop=dict(eos_ids=[0]), logprobs=2, constraint=tries([31]), guidance=GUIDE)
    bare = full.without_selection()
    assert not bare.select and full.select
    assert (bare.proc, bare.stop, bare.n_top, bare.cons, bare.guidance) == (None,) * 5 and not bare.rewrites_logits
    assert bare.graph_key(False) == plan().without_selection().graph_key(False)       # one teacher-forced step, whatever the call
    assert bare.graph_key(False) != plan().graph_key(False)


def test_a_plan_passes_through_unchanged():
    p = plan(sampling=SAMPLED, processors=procs([11, 12]), logprobs=1)
    assert LMEngine.selection_plan(p) is p and LMEngine.selection_plan(plan=p, vocab=V) is p
    with pytest.raises(ValueError):
        LMEngine.selection_plan(p, sampling=SAMPLED)            # a plan AND keywords: which one holds?


def test_plans_are_immutable():
    p = plan(logprobs=1)
    with pytest.raises(AttributeError):
        p.n_top = 2


@pytest.mark.parametrize("kw", [dict(stop=dict(eos_ids=[0, 7])), dict(logprobs=0), dict(constraint=tries([31])), dict(guidance=GUIDE)],
                         ids=["stop", "logprobs", "constraint", "guidance"])
def test_refused_with_beam(kw):
    with pytest.raises(NotImplementedError, match="not combined with beam search"):
        plan(beam=BEAM, **kw)
    assert plan(**kw) is not None and plan(beam=BEAM, processors=procs([11])).is_beam        # each alone, and what beam does take


@pytest.mark.parametrize("p,c,g", list(itertools.product((False, True), repeat=3)))
def test_rewrites_logits(p, c, g):
    made = plan(processors=procs([11]) if p else None, constraint=tries([31]) if c else None, guidance=GUIDE if g else None)
    assert made.rewrites_logits is (p or c or g)
    assert (made.proc is not None, made.cons is not None, made.guidance is not None) == (p, c, g)


def test_the_normalisers_check_as_before():
    assert plan(sampling=None).mode is None and plan(sampling=(0.7, 5.0, 1)).mode == (0.7, 5, 1.0)
    assert plan(processors=dict(repetition_penalty=1.0)).proc is None                # the defaults: nothing is launched
    with pytest.raises(ValueError):
        plan(sampling=("warp", 0.7, 5))
    with pytest.raises(ValueError):
        plan(logprobs=21)
    with pytest.raises(ValueError):
        plan(logprobs=True)
    with pytest.raises(ValueError):
        plan(logprobs=3, vocab=2)                     # more alternatives than logits
    with pytest.raises(ValueError):
        plan(guidance=(-1.0, 0.0))
    with pytest.raises(ValueError):
        plan(processors=procs([11], repetition_penalty=0.0))
    with pytest.raises(ValueError):
        plan(stop=dict(eos_ids=[]))


# ---- arm(): preconditions, vocabulary range, copies only when the contents differ -- on a host-memory cache -------------------------
class _State:
    def __init__(self, B):
        self.logits, self.logits_proc, self.graphs = torch.zeros(B, 64), None, {}


def _cache(B=2, ragged=False):
    cache = KVCache(1, B, 1, 8, "cpu", ragged=ragged)
    cache.decode_state = _State(B)
    return cache, cache.decode_state


def test_arm_refuses_a_step_on_a_cache_that_was_not_armed():
    cache, st = _cache()
    with pytest.raises(ValueError, match="needs a cache armed for it"):
        plan(stop=dict(eos_ids=[0, 7])).arm(cache, st)
    with pytest.raises(ValueError, match="beam decoding needs a cache armed for this num_beams"):
        plan(beam=BEAM).arm(cache, st)
    with pytest.raises(ValueError, match="beam decoding needs a cache armed for this num_beams"):
        plan(beam=BEAM).without_selection().arm(cache, st)
    plan().without_selection().arm(cache, st)
    assert cache.stop_table is None and cache.suppress is None and cache.lp is None and cache.trie_table is None


def test_arm_checks_the_vocabulary_range():
    cache, st = _cache()
    for bad in (dict(processors=procs([V])), dict(stop=dict(eos_ids=[0, V])), dict(stop=dict(eos_ids=[0], stop_seqs=[[5, V + 1]])),
                dict(constraint=tries([31, V]))):
        with pytest.raises(ValueError):
            plan(**bad).arm(cache, st, first=True)
    with pytest.raises(ValueError, match="the constraint has 2 rows, the cache 3"):
        plan(constraint=tries([31])).arm(*_cache(3), first=True)


def test_arm_copies_only_what_differs():
    cache, st = _cache()
    a = plan(processors=procs([11, 12]), stop=dict(eos_ids=[0, 7], stop_seqs=[[21, 22]]), constraint=tries([31, 32]), logprobs=3)
    a.arm(cache, st, first=True)
    assert cache.suppress[:2].tolist() == [11, 12] and cache.stop_table[:2].tolist() == [0, 7]
    assert cache.finish.tolist() == [[-1, 0]] * 2 and cache.trie_held is a.cons and cache.top_id.shape == (2, 8, 3)
    assert st.logits_proc is not None and st.logits_proc.shape == st.logits.shape           # processors AND log-probabilities
    held = (cache.suppress, cache.stop_table, cache.trie_table, cache.lp, st.logits_proc)
    cache.finish[0, 0] = 4                                                                   # row 0 finished at step 4
    cache.suppress[:2] = 99                                                                  # (would be rewritten by a copy)
    a.arm(cache, st)
    same = plan(processors=procs([11, 12]), stop=dict(eos_ids=[0, 7], stop_seqs=[[21, 22]]), constraint=tries([31, 32]), logprobs=3)
    same.arm(cache, st)
    assert cache.suppress[:2].tolist() == [99, 99] and cache.trie_held is a.cons            # equal contents: nothing copied
    assert cache.finish[0].tolist() == [4, 0]                                                # a step leaves the record alone
    other = plan(processors=procs([13, 14]), stop=dict(eos_ids=[0, 9], stop_seqs=[[23, 24]]), constraint=tries([41], [42]), logprobs=3)
    other.arm(cache, st)
    assert cache.suppress[:2].tolist() == [13, 14] and cache.stop_table[:2].tolist() == [0, 9] and cache.trie_held is other.cons
    assert all(x is y for x, y in zip(held, (cache.suppress, cache.stop_table, cache.trie_table, cache.lp, st.logits_proc)))
    other.arm(cache, st, first=True)
    assert cache.finish.tolist() == [[-1, 0]] * 2                                            # the first call of a loop resets it


def test_arm_allocates_the_second_buffer_only_with_a_rewriter():
    cache, st = _cache(ragged=True)            # (a guided cache: one position per row, R pairs)
    plan(logprobs=2).arm(cache, st)
    assert st.logits_proc is None and cache.top_lp.shape == (2, 8, 2)
    plan(guidance=GUIDE, logprobs=2).arm(cache, st)
    assert st.logits_proc is not None
    with pytest.raises(ValueError, match="guidance needs a ragged cache of 2R rows"):
        plan(guidance=GUIDE).arm(*_cache())


def test_the_cache_drops_graphs_by_the_keys_fields():
    cache, st = _cache()
    keys = {n: p.graph_key(True) for n, p in dict(plain=plan(), cons=plan(constraint=tries([31])), lp=plan(logprobs=3),
                                                  both=plan(constraint=tries([31]), logprobs=3), beam=plan(beam=BEAM)).items()}
    plan(constraint=tries([31]), logprobs=3).arm(cache, st)
    st.graphs.update({k: n for n, k in keys.items()})
    cache.alloc_logprobs(3)
    cache.alloc_trie(cache.trie_table.numel())
    assert len(st.graphs) == 5                                     # buffers that fit: every step stays
    cache.alloc_logprobs(5)
    assert sorted(st.graphs.values()) == ["beam", "cons", "plain"]
    st.graphs.update({k: n for n, k in keys.items()})
    cache.alloc_trie(cache.trie_table.numel() + 1)
    assert sorted(st.graphs.values()) == ["beam", "lp", "plain"]
