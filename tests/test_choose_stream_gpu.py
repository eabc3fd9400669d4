"""Choosing over a request stream on the engine (DESIGN.md "Choosing over a request stream"): choose_stream on the reduced model
of tests/test_continue_generate_gpu.py.  Scheduling changes nothing, exactly: every request's choice, tokens, reason and the
BITS of its log-probabilities and top lists equal those of a static ``choose(..., lengths=...)`` over batches of three of the
same requests padded to the session's staging shape, one trie per row -- whatever ``every``, the order of the requests and the
number of turns of the ring are; with a prefix, those of the static call continued from the expanded prefix cache.

The answer sets are built from every request's own plain greedy ids, so that the walks go deep: single-token sets, sets whose
members share prefixes, sets with a choice that is a proper prefix of another, sets that lack the request's greedy first token,
and one TokenTrie OBJECT shared by four requests.  The choice seed is CHOICE_SEED = 1: the first of range(8) under which the
preconditions of ``case`` hold on the reference alone (seed 0 ends no request at the inner terminal; the fixture searches in
that order and asserts which one it took)."""
import pytest
import torch

from test_continue_generate_gpu import embeds, model, oracle  # noqa: F401  (fixtures)
from test_stream_gpu import LENS, MAX_PROMPT, ORDERS, S_STAGE, SLOTS, sessions, static_batches  # noqa: F401

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
MAX_CHOICE = 6
N_TOP = 3
PROMPT_SEED, CHOICE_SEED = 21, 1
SHARED = (1, 4, 6, 9)               # the requests that pass one TokenTrie object
INNER = (0, 2, 5)                   # the requests whose first choice is a proper prefix of their second


def answer_sets(plain, eos, V, seed):
    """Per request its choices (lists of id lists, or the shared TokenTrie) from the plain greedy ids of all requests."""
    from magma_amd.sampling import TokenTrie
    g = torch.Generator().manual_seed(1000 + seed)

    def other(n, avoid):
        out = []
        while len(out) < n:
            t = int(torch.randint(0, V, (1,), generator=g))
            if t != eos and t not in avoid and t not in out:
                out.append(t)
        return out

    clean = [[t for t in ids if t != eos] for ids in plain]
    assert all(len(c) >= 6 for c in clean)
    shared = TokenTrie([clean[i][:3] for i in SHARED[:2]] + [clean[SHARED[2]][:2] + other(1, ())] + [clean[SHARED[3]][:1] + other(1, ())] +
                       [other(2, [c[0] for c in clean])])
    sets = []
    for i, p in enumerate(clean):
        a = other(6, p)
        if i in SHARED:
            sets.append(shared)
        elif i in INNER:            # [p0 p1] is listed and is an inner node: eos competes with one unlikely continuation
            sets.append([p[:2], p[:2] + a[:1], p[:2] + a[:1] + a[1:2], a[2:4]])
        elif i == 3:                # single tokens without the greedy one
            sets.append([[t] for t in a])
        elif i == 7:                # deep, with shared prefixes
            sets.append([p[:5], p[:4] + a[:1], p[:2] + a[1:3], p[:1], a[3:6]])
        else:                       # another request's walk: the first token is not this request's greedy one
            q = clean[(i + 1) % len(clean)]
            sets.append([q[:4], q[:2] + a[:2], a[2:5]] if q[0] != p[0] else [a[:3], a[3:5]])
    return sets


def static_choose(model, prompts, tries, rows=None, **kw):  # noqa: F811
    """choose() over batches of three of the requests ``rows`` (default: all, in order; a last batch is filled with a one-row
    prompt under the first trie), each padded to S_STAGE rows: {request: (choice, tokens, lp, top ids, top lp)}."""
    from magma_amd.sampling import choose
    rows = list(range(len(prompts))) if rows is None else rows
    d, out = prompts[0].shape[1], {}
    for at in range(0, len(rows), 3):
        group = rows[at:at + 3]
        emb = torch.zeros(3, S_STAGE, d, dtype=BF16, device=model.device)
        lens, row_tries = [1, 1, 1], [tries[group[0]]] * 3
        for r, i in enumerate(group):
            emb[r, : prompts[i].shape[0]], lens[r], row_tries[r] = prompts[i], prompts[i].shape[0], tries[i]
        past = {} if "cache" not in kw else dict(past_key_values=kw["cache"].expand(3))
        index, lp = choose(model, emb, row_tries, lengths=lens, eos_token=[model.eos_token], top_logprobs=N_TOP, **past)
        for r, i in enumerate(group):
            n = int(lp.count[r])
            out[i] = (int(index[r]), lp.tokens[r, :n].tolist(), lp.logprobs[r, :n].clone(), lp.top_ids[r, :n].clone(),
                      lp.top_logprobs[r, :n].clone())
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def same(got, want, n_top=N_TOP):
    """A StreamChoice against a reference entry, log-probabilities by their bits."""
    ok = (got.choice, got.tokens.tolist(), got.reason) == (want[0], want[1], "eos") and torch.equal(bits(got.logprobs), bits(want[2]))
    if n_top:
        ok = ok and torch.equal(got.top_ids, want[3]) and torch.equal(bits(got.top_logprobs), bits(want[4]))
    return ok and got.top_ids.shape == (len(want[1]), n_top) and got.top_logprobs.shape == (len(want[1]), n_top)


def preconditions(model, prompts, plain, tries, ref):  # noqa: F811
    """On the reference alone; returns what fails (empty: all hold)."""
    eos, fails = model.eos_token, []
    if sum(len(ref[i][1]) - 1 >= 3 for i in ref) < 3:
        fails.append("three requests must answer with three or more tokens")
    if sum(ref[i][1][0] != plain[i][0] for i in ref) < 3:
        fails.append("three requests must answer with a first token that is not their greedy first token")
    if not any(i in INNER and len(ref[i][1]) == 3 and ref[i][1][-1] == eos for i in ref):
        fails.append("a request must end at the inner terminal")
    if min(ref[i][0] for i in ref) < 0 or not all(ref[i][1][-1] == eos for i in ref):
        fails.append("every answer is a listed choice and ends with eos")
    return fails


@pytest.fixture(scope="module")
def case(model):  # noqa: F811
    """(prompts, tries per request, the reference) -- computed once, shared and left unchanged."""
    from magma_amd.sampling import TokenTrie
    prompts = embeds(model, LENS, seed=PROMPT_SEED)
    plain = [r[0] for r in static_batches(model, prompts, eos_token=-7)]
    V, tried = model.lm.engine.V, {}
    for seed in range(8):
        sets = answer_sets(plain, model.eos_token, V, seed)
        tries = [s if isinstance(s, TokenTrie) else TokenTrie(s) for s in sets]
        ref = static_choose(model, prompts, tries)
        tried[seed] = preconditions(model, prompts, plain, tries, ref)
        if not tried[seed]:
            break
    print(f"choice seed {seed}; rejected: {tried}")
    assert not tried[seed] and seed == CHOICE_SEED, tried
    assert len({id(t) for t in tries}) == len(tries) - 3 and max(t.max_len() for t in tries) <= MAX_CHOICE
    # permuting the rows of a static batch permutes tokens and log-probability bits
    perm = static_choose(model, prompts, tries, rows=[7, 2, 0])
    assert all(perm[i][:2] == ref[i][:2] and all(torch.equal(bits(a), bits(b)) for a, b in zip(perm[i][2:], ref[i][2:])) for i in perm)
    return prompts, sets, tries, ref


def stream(model, prompts, sets, order=None, **kw):  # noqa: F811
    """choose_stream over the requests in ``order``: {request: StreamChoice}, every request exactly once."""
    order = list(range(len(prompts))) if order is None else order
    kw = {**dict(slots=SLOTS, max_choice_tokens=MAX_CHOICE, max_prompt=MAX_PROMPT, eos_token=[model.eos_token], top_logprobs=N_TOP), **kw}
    got = list(model.choose_stream([(prompts[i] if i % 2 else prompts[i][None], sets[i]) for i in order], **kw))
    assert sorted(r.index for r in got) == list(range(len(order))), [r.index for r in got]
    assert all(0 <= r.slot < kw["slots"] and r.tokens.dtype == torch.int64 and r.tokens.device.type == "cpu" for r in got)
    return {order[r.index]: r for r in got}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("every", [1, 4, 8])
def test_scheduling_changes_nothing(model, case, sessions, every, order):  # noqa: F811
    prompts, sets, tries, ref = case
    res = stream(model, prompts, sets, ORDERS[order], every=every)
    for i in ref:
        assert same(res[i], ref[i]), (i, res[i], ref[i])
    ses, = sessions
    assert ses.steps % every == 0 and all(o is None for o in ses.occ) and all(t is None for t in ses.slot_trie)
    assert len({r.slot for r in res.values()}) == SLOTS


def test_the_ring_wraps_and_top_logprobs_zero(model, case, sessions):  # noqa: F811
    """The requests five times over through an 8-column ring (7 budget + every = 1): many turns, windows across the wrap; and
    without alternatives."""
    prompts, sets, tries, ref = case
    order = (ORDERS["shuffled"] + ORDERS["forward"] + ORDERS["reversed"]) * 2
    kw = dict(slots=SLOTS, max_choice_tokens=MAX_CHOICE, max_prompt=MAX_PROMPT, eos_token=[model.eos_token], every=1)
    got = list(model.choose_stream([(prompts[i], sets[i]) for i in order], top_logprobs=0, **kw))
    assert sorted(r.index for r in got) == list(range(len(order)))
    for r in got:
        assert same(r, ref[order[r.index]], n_top=0), r
    ses, = sessions
    assert ses.Hc == 8 and ses.steps > 4 * ses.Hc, (ses.Hc, ses.steps)
    wrapped = sum(1 for r in got if len(r.tokens) >= 3)
    assert wrapped >= 12


def test_admit_rows_one_is_schedule_invariant(model, case):  # noqa: F811
    """One request per admission prefill (another staging shape than the reference's: compared among themselves)."""
    prompts, sets, tries, ref = case
    runs = [stream(model, prompts, sets, ORDERS[o], every=e, admit_rows=1) for e, o in ((1, "forward"), (4, "reversed"), (8, "shuffled"))]
    for i in ref:
        assert same(runs[1][i], (runs[0][i].choice, runs[0][i].tokens.tolist(), runs[0][i].logprobs, runs[0][i].top_ids, runs[0][i].top_logprobs))
        assert same(runs[2][i], (runs[0][i].choice, runs[0][i].tokens.tolist(), runs[0][i].logprobs, runs[0][i].top_ids, runs[0][i].top_logprobs))
    assert sum(runs[0][i].choice == ref[i][0] for i in ref) >= len(ref) - 2


@pytest.mark.parametrize("shared", [False, True])
def test_a_session_prefix(model, case, shared):  # noqa: F811
    """prefix=: the static choose() continued from the expanded prefix cache.  share_prefix=True sums the attention in another
    order: the session against itself under two schedules, and choices equal to the unshared reference but for near-ties."""
    prompts, sets, tries, _ = case
    prefix = embeds(model, [37], seed=77)[0]
    cache = model.cache_prompt(prefix[None])
    ref = static_choose(model, prompts, tries, cache=cache)
    if not shared:
        for form, every, order in ((cache, 4, "shuffled"), (prefix, 1, "forward")):
            res = stream(model, prompts, sets, ORDERS[order], every=every, prefix=form)
            for i in ref:
                assert same(res[i], ref[i]), (i, res[i], ref[i])
    else:
        a = stream(model, prompts, sets, ORDERS["forward"], every=1, prefix=cache, share_prefix=True)
        b = stream(model, prompts, sets, ORDERS["shuffled"], every=8, prefix=cache, share_prefix=True)
        for i in ref:
            assert same(b[i], (a[i].choice, a[i].tokens.tolist(), a[i].logprobs, a[i].top_ids, a[i].top_logprobs)), i
        assert sum(a[i].choice == ref[i][0] for i in ref) >= len(ref) - 2
    assert cache.expand(2).rows_pos().tolist() == [37, 37]


def test_poisoned_idle_memory_changes_nothing(model, case, monkeypatch):  # noqa: F811
    """Between rounds: NaN into the K / V of idle slots and of every position at or past a live row's write position, into the
    staging cache, and into the log-probability rows and path caches of idle slots."""
    from magma_amd.engine import SlotSession
    prompts, sets, tries, ref = case
    harvest, rounds = SlotSession._harvest, []

    def poisoned(self):
        out = harvest(self)
        for b, o in enumerate(self.occ):
            at = 0 if o is None else o[2] + (self.steps - o[4])
            self.cache.k[:, b, :, at:] = float("nan")
            self.cache.v[:, b, :, at:] = float("nan")
            if o is None:
                self.cache.lp[b], self.cache.top_lp[b] = float("nan"), float("nan")
                self.cache.top_id[b], self.cache.trie_path[b], self.cache.trie_roots[b] = -7, 10 ** 6, 10 ** 6
        self.roots_held = None          # (the poisoned roots of idle slots are rewritten at the next admission)
        self.stage.k.fill_(float("nan"))
        self.stage.v.fill_(float("nan"))
        rounds.append(sum(o is None for o in self.occ))
        return out

    monkeypatch.setattr(SlotSession, "_harvest", poisoned)
    res = stream(model, prompts, sets, ORDERS["shuffled"], every=4)
    for i in ref:
        assert same(res[i], ref[i]), (i, res[i], ref[i])
    assert len(rounds) > 4 and max(rounds) >= 1


def test_two_sessions_and_plain_calls_interleaved(model, case):  # noqa: F811
    from magma_amd.sampling import generate
    prompts, sets, tries, ref = case
    plain_in = embeds(model, [9, 30], seed=24)

    def plain():
        return generate(model, plain_in, max_steps=6, temperature=0.0, eos_token=-7, decode=False)

    want_plain = plain()
    kw = dict(slots=SLOTS, max_choice_tokens=MAX_CHOICE, max_prompt=MAX_PROMPT, eos_token=[model.eos_token], top_logprobs=N_TOP)
    orders = (ORDERS["forward"], ORDERS["reversed"])
    its = [model.choose_stream([(prompts[i], sets[i]) for i in orders[0]], every=4, **kw),
           model.choose_stream([(prompts[i], sets[i]) for i in orders[1]], every=1, **kw)]
    got, live, turn = [{}, {}], [True, True], 0
    while any(live):
        s = turn % 2
        turn += 1
        if live[s]:
            r = next(its[s], None)
            if r is None:
                live[s] = False
            else:
                got[s][orders[s][r.index]] = r
        if turn % 3 == 0:
            assert torch.equal(plain(), want_plain)
    for g in got:
        for i in ref:
            assert same(g[i], ref[i]), (i, g[i], ref[i])
    assert torch.equal(plain(), want_plain)


def test_a_trie_that_outgrows_the_capacity_mid_session(model, case, sessions):  # noqa: F811
    """Request 3 of the stream brings a trie of ~1500 single-token choices (and its own choices): the table outgrows the 4096
    entries it was allocated with, is re-allocated, the captured step with it, and nobody's answer changes."""
    from magma_amd.sampling import TokenTrie
    prompts, sets, tries, ref = case
    eos, V = model.eos_token, model.lm.engine.V
    own = sets[3]
    listed = {tuple(c) for c in own}
    big = own + [[t] for t in range(V) if t != eos and (t,) not in listed][:1500]
    assert TokenTrie(big).flat().numel() > 4096
    order = ORDERS["forward"]
    mixed = [big if i == 3 else sets[i] for i in range(len(sets))]
    ses_tables = []
    it = model.choose_stream([(prompts[i], mixed[i]) for i in order], slots=SLOTS, max_choice_tokens=MAX_CHOICE, max_prompt=MAX_PROMPT,
                             eos_token=[eos], top_logprobs=N_TOP, every=2, trie_capacity=4096)
    res = {}
    for r in it:
        res[order[r.index]] = r
        ses_tables.append(sessions[0].cache.trie_table)
    assert ses_tables[0].numel() == 4096 and ses_tables[-1].numel() > 4096
    wide = static_choose(model, prompts, [TokenTrie(big) if i == 3 else tries[i] for i in range(len(tries))], rows=[3, 4, 5])
    for i in ref:
        assert same(res[i], wide[3] if i == 3 else ref[i]), (i, res[i])


def test_the_slot_step_has_the_launches_of_the_per_row_step(model, case, monkeypatch):  # noqa: F811
    """Eager steps, counted on the ops module: a slot step under the constraint with log-probabilities makes as many selection
    launches as generate()'s per-row step under them -- constraint, selection, log-probabilities, bookkeeping."""
    from magma_amd import ops
    from magma_amd.engine import SlotSession
    from magma_amd.sampling import choose
    prompts, sets, tries, ref = case
    eng = model.lm.engine
    orig = eng.decode
    monkeypatch.setattr(eng, "decode", lambda *x, **kw: orig(*x, **{**kw, "use_graph": False}))
    names = ("logits_process", "logits_process_constrained", "logits_process_slots", "logits_process_constrained_slots", "argmax",
             "token_logprobs", "token_logprobs_slots", "sample_finish", "sample_finish_rows", "sample_finish_slots")
    calls, inside = [], [False]
    for n in names:
        monkeypatch.setattr(ops, n, lambda *a, _n=n, _f=getattr(ops, n), **k: (calls.append(_n) if inside[0] else None, _f(*a, **k))[1])
    step = SlotSession._step

    def counted(self):
        inside[0] = True
        try:
            step(self)
        finally:
            inside[0] = False

    monkeypatch.setattr(SlotSession, "_step", counted)
    res = stream(model, prompts[:3], sets[:3], every=1)
    n_steps = max(len(r.tokens) for r in res.values()) - 1
    slot_calls = list(calls)
    per_step = ["logits_process_constrained_slots", "argmax", "token_logprobs_slots", "sample_finish_slots"]
    assert slot_calls[: len(per_step)] == per_step and len(slot_calls) % len(per_step) == 0 and len(slot_calls) >= n_steps * len(per_step)
    # generate()'s per-row step: everything after the first token's selection
    calls.clear()
    inside[0] = True
    emb = torch.zeros(3, S_STAGE, prompts[0].shape[1], dtype=BF16, device=model.device)
    for r in range(3):
        emb[r, : prompts[r].shape[0]] = prompts[r]
    choose(model, emb, tries[:3], lengths=[p.shape[0] for p in prompts[:3]], eos_token=[model.eos_token], top_logprobs=N_TOP)
    inside[0] = False
    flat_step = ["logits_process_constrained", "argmax", "token_logprobs", "sample_finish_rows"]
    assert calls[: len(flat_step)] == flat_step and len(calls) % len(flat_step) == 0
    assert len(per_step) == len(flat_step)
    for i in range(3):
        assert same(res[i], ref[i])


def test_errors_leave_the_earlier_requests_whole(model, case):  # noqa: F811
    prompts, sets, tries, ref = case
    kw = dict(slots=SLOTS, max_choice_tokens=MAX_CHOICE, max_prompt=MAX_PROMPT, eos_token=[model.eos_token], top_logprobs=N_TOP, every=2)
    long = [list(range(1, MAX_CHOICE + 2))]
    it = model.choose_stream([(prompts[i], sets[i]) for i in (3, 1, 0, 5)] + [(prompts[2], long), (prompts[2], sets[2])], **kw)
    got = []
    with pytest.raises(ValueError, match="request 4"):
        for r in it:
            got.append(r)
    assert sorted(r.index for r in got) == [0, 1, 2, 3]
    for r in got:
        assert same(r, ref[(3, 1, 0, 5)[r.index]]), r
    res = stream(model, prompts, sets, every=8)                  # the engine is as usable as before
    assert all(same(res[i], ref[i]) for i in ref)
