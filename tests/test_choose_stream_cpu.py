"""Choosing over a request stream on the host (DESIGN.md "Choosing over a request stream"): the statement of the window the slot
kernels read (magma_amd.sampling.slot_tokens) at its boundaries, choose_stream's argument checks, its host loop -- one solo
choose() per request -- over the tiny random GPT-J of tests/test_stream_cpu.py, and the slot plan with a constraint, rules and
log-probabilities.  No GPU: the kernels are tested in tests/test_stream_rules_kernels_gpu.py, the session in
tests/test_choose_stream_gpu.py."""
import pytest
import torch

from magma_amd.sampling import StreamChoice, TokenTrie, choose, choose_stream, slot_tokens, slot_update
from test_beam_search_cpu import EOS, V, _tiny_gptj
from test_logits_processors_cpu import _HostMagma
from test_stream_cpu import _NoModel


def test_slot_tokens_at_its_boundaries():
    cols = 8
    ring = torch.arange(100, 100 + cols)
    # n = 1: the admission wrote the first token at column (step - 1) % cols = begin
    assert slot_tokens(ring, 3, 4, cols).tolist() == [103]
    assert slot_tokens(ring, 3, 4 + 5 * cols, cols).tolist() == [103]           # the session's step counter only enters mod cols
    assert slot_tokens(ring, 0, 1, cols).tolist() == [100] and slot_tokens(ring, 7, 8, cols).tolist() == [107]
    # a window inside the ring, and one that reaches the last column exactly
    assert slot_tokens(ring, 2, 6, cols).tolist() == [102, 103, 104, 105]
    assert slot_tokens(ring, 5, 8, cols).tolist() == [105, 106, 107]
    # across the wrap: begin 6, newest column 1
    assert slot_tokens(ring, 6, 10, cols).tolist() == [106, 107, 100, 101]
    # n = cols: the whole ring, from begin on -- newest column begin - 1
    assert slot_tokens(ring, 3, 3 + cols, cols).tolist() == [103, 104, 105, 106, 107, 100, 101, 102]
    assert slot_tokens(ring, 0, cols, cols).tolist() == list(range(100, 108))
    # step <= 0 (before any step): the column is still formed mod cols, as the admission kernel forms it
    assert slot_tokens(ring, 7, 0, cols).tolist() == [107]
    for begin in (-1, cols):
        with pytest.raises(ValueError):
            slot_tokens(ring, begin, 4, cols)
    with pytest.raises(ValueError):
        slot_tokens(ring[:4], 0, 4, cols)


def test_slot_tokens_counts_as_slot_update_counts():
    """The count is slot_update's at the step before: a row whose budget is n finishes (length) exactly at the step after which
    slot_tokens returns n tokens."""
    cols, begin = 8, 5
    ring = torch.arange(cols)[None]
    for n in range(1, cols + 1):
        step = begin + n - 1                    # the step that wrote the n-th token
        done, _ = slot_update(ring, step, torch.zeros(1, dtype=torch.bool), [begin], [n], [99])
        early, _ = slot_update(ring, step, torch.zeros(1, dtype=torch.bool), [begin], [n + 1], [99])
        assert bool(done[0]) and not bool(early[0])
        assert slot_tokens(ring[0], begin, step + 1, cols).numel() == n


def _requests(seed=11):
    g = torch.Generator().manual_seed(seed)
    prompts = [torch.randn(1, n, 32, generator=g) if i % 2 else torch.randn(n, 32, generator=g) for i, n in enumerate((5, 1, 7, 3, 5, 2))]
    shared = TokenTrie([[7, 8], [7, 9, 10], [11]])
    sets = [[[4, 5, 6], [4, 5], [9]], shared, [[12]], shared, [[3 + i] for i in range(6)], [[20, 21, 22, 23], [20, 30]]]
    return prompts, sets


def test_host_loop_equals_solo_choose_per_request():
    model = _HostMagma(_tiny_gptj(seed=4, eos_bias=1.5))
    prompts, sets = _requests()
    pulled = []

    def stream():
        for i, item in enumerate(zip(prompts, sets)):
            pulled.append(i)
            yield item

    it = choose_stream(model, stream(), max_choice_tokens=4, max_prompt=8, top_logprobs=2, eos_token=[EOS, V - 3])
    assert pulled == []                                      # nothing runs before the first next()
    got = []
    for res in it:
        assert isinstance(res, StreamChoice) and pulled == list(range(res.index + 1))
        got.append(res)
    assert [r.index for r in got] == list(range(len(prompts)))
    for r, p, c in zip(got, prompts, sets):
        index, lp = choose(model, p.view(1, -1, 32), c, eos_token=[EOS, V - 3], top_logprobs=2)
        n = int(lp.count[0])
        assert r.choice == int(index[0]) and r.slot is None and r.reason == "eos"
        assert r.tokens.dtype == torch.int64 and r.tokens.tolist() == lp.tokens[0, :n].tolist() and r.tokens[-1] in (EOS, V - 3)
        assert torch.equal(r.logprobs, lp.logprobs[0, :n]) and torch.equal(r.top_ids, lp.top_ids[0, :n])
        assert torch.equal(r.top_logprobs, lp.top_logprobs[0, :n]) and r.top_ids.shape == (n, 2)
        trie = c if isinstance(c, TokenTrie) else TokenTrie(c)
        assert trie.index(r.tokens.tolist()[:-1]) == r.choice
    assert len({r.choice for r in got}) > 1 and max(len(r.tokens) for r in got) >= 3


def test_rules_and_prefix_reach_the_solo_calls():
    model = _HostMagma(_tiny_gptj(seed=4, eos_bias=1.5))
    prompts, sets = _requests()
    prefix = torch.randn(3, 32, generator=torch.Generator().manual_seed(2))
    kw = dict(repetition_penalty=1.4, min_new_tokens=1)
    got = list(choose_stream(model, zip(prompts, sets), max_choice_tokens=4, max_prompt=8, prefix=prefix, **kw))
    for r, p, c in zip(got, prompts, sets):
        index, lp = choose(model, torch.cat([prefix, p.view(-1, 32)])[None], c, **kw)
        assert r.choice == int(index[0]) and r.tokens.tolist() == lp.tokens[0, : int(lp.count[0])].tolist()
        assert r.top_ids.shape == (len(r.tokens), 0)


def test_argument_checks():
    reqs = [(torch.zeros(2, 8), [[1, 2]])]
    for kw in [dict(slots=17), dict(slots=0), dict(admit_rows=0), dict(slots=4, admit_rows=5), dict(every=0), dict(max_choice_tokens=0),
               dict(max_choice_tokens=65), dict(max_choice_tokens=2.0), dict(max_prompt=0), dict(max_prompt=250, max_choice_tokens=7),
               dict(eos_token=[EOS, V]), dict(eos_token=list(range(9))), dict(top_logprobs=21), dict(top_logprobs=-1),
               dict(trie_capacity=0), dict(trie_capacity=1.5), dict(repetition_penalty=0.0), dict(min_new_tokens=-1),
               dict(suppress_tokens=[V]), dict(share_prefix=True), dict(share_prefix=1), dict(prefix=torch.zeros(2, 3, 8))]:
        with pytest.raises(ValueError):
            choose_stream(_NoModel(), reqs, **kw)
    for kw in [dict(temperature=0.7), dict(stop_sequences=[[1]]), dict(no_repeat_ngram_size=2), dict(max_new_tokens=4)]:
        with pytest.raises(TypeError):      # selection is greedy, the budget is the choices'
            choose_stream(_NoModel(), reqs, **kw)
    with pytest.raises(TypeError):          # keyword-only
        choose_stream(_NoModel(), reqs, 8)


def test_a_failing_request_raises_after_the_earlier_ones_were_yielded():
    model = _HostMagma(_tiny_gptj(seed=4, eos_bias=1.5))
    ok = torch.randn(3, 32, generator=torch.Generator().manual_seed(1))
    good = [[5, 6], [7]]
    bad_items = [(torch.randn(9, 32), good), (ok, [[1, 2, 3, 4, 5]]), (ok, []), (ok, [[V]]), (ok, "text"), ok, (ok, good, 3),
                 (torch.zeros(2, 3, 32), good), (ok, [good, good])]
    for bad in bad_items:
        it = choose_stream(model, [(ok, good), bad, (ok, good)], max_choice_tokens=4, max_prompt=8)
        first = next(it)
        assert first.index == 0 and first.choice in (0, 1)
        with pytest.raises(ValueError, match="request 1"):
            next(it)
    # the rules are checked against every request's own choices, as generate(constraint=...) checks them
    for kw, bad in [(dict(min_new_tokens=2), [[7]]), (dict(suppress_tokens=[9]), [[9], [8]])]:
        it = choose_stream(model, [(ok, [[5, 6]]), (ok, bad)], max_choice_tokens=4, max_prompt=8, **kw)
        assert next(it).index == 0
        with pytest.raises(ValueError, match="request 1"):
            next(it)


def test_slot_plan_takes_constraint_rules_and_logprobs():
    from magma_amd.selection import SlotConstraint, TokenSelection
    stop = dict(eos_ids=(EOS,), stop_seqs=())
    plan = TokenSelection.selection_plan(stop=stop, constraint=True, logprobs=3, vocab=V, slots=True,
                                         processors=dict(repetition_penalty=1.2, min_new_tokens=1))
    assert plan.slots and isinstance(plan.cons, SlotConstraint) and plan.n_top == 3 and plan.proc[:3] == (1.2, 0, 1)
    assert plan.second_buffer and plan.rewrites_logits
    key = plan.graph_key(True)
    assert key.slots and key.constrained and key.n_top == 3 and key.proc == (1.2, 0, 1, 0) and key._fields[-1] == "slots"
    bare = TokenSelection.selection_plan(stop=stop, vocab=V, slots=True)
    assert bare.cons is None and bare.n_top is None and bare.graph_key(True) != key
    assert TokenSelection.selection_plan(stop=stop, logprobs=0, vocab=V, slots=True).n_top == 0
    # what a slot plan still refuses, and the constraint forms that belong to the other kind of plan
    for kw in [dict(beam=(2, 1.0, False, 8)), dict(contrast=(4, 0.6)), dict(guidance=(1.5, 0.0))]:
        with pytest.raises(NotImplementedError, match="not combined with it yet"):
            TokenSelection.selection_plan(stop=stop, vocab=V, slots=True, **kw)
    with pytest.raises(NotImplementedError):
        TokenSelection.selection_plan(vocab=V, slots=True)           # no per-row stopping
    with pytest.raises(ValueError):
        TokenSelection.selection_plan(stop=stop, vocab=V, slots=True, constraint=[TokenTrie([[1]])])
    with pytest.raises(ValueError):
        TokenSelection.selection_plan(stop=stop, vocab=V, constraint=True)


def test_a_stale_library_names_the_missing_symbol(tmp_path, monkeypatch):
    """lib.load() against a library of the same C-ABI revision that lacks an entry point this package binds: the message names
    the symbol and says rebuild.  (A stand-in library: every other symbol is there, the revision is the bound one.)"""
    from magma_amd import lib

    class _Symbol:
        restype = argtypes = None

        def __call__(self):
            return lib.ABI_VERSION

    class _Stale:
        def __getattr__(self, name):
            if name == "mg_token_logprobs_slots_f32":
                raise AttributeError(name)
            return _Symbol()

    stale = tmp_path / "libmagma_hip.so"
    stale.write_bytes(b"")
    monkeypatch.setenv("MAGMA_HIP_LIB", str(stale))
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib.C, "CDLL", lambda path: _Stale())
    with pytest.raises(lib.MagmaHipError, match=r"mg_token_logprobs_slots_f32.*rebuild"):
        lib.load()
    assert lib._lib is None
