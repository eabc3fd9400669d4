"""Request streams on the engine (DESIGN.md "Request streams"): generate_stream on the reduced model of
tests/test_continue_generate_gpu.py (the oracle's seed-11 weights, adapters x 20).  Scheduling changes nothing, exactly: every
request's tokens, reason and index equal those of a static ragged generate() over batches of three of the same requests, whatever
``every``, the order of the requests and the admission width are; sampling at top_k = 1 is greedy; NaN in everything a live row
must not read changes nothing; the quantised and the unpacked token steps are schedule-invariant; two sessions and plain
generate() calls on one engine do not disturb each other; the error cases."""
import pytest
import torch

from test_continue_generate_gpu import embeds, model, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LENS = [1, 7, 40, 3, 64, 12, 65, 5, 33, 2, 19]
LIMITS = [1, 2, 9, 20, 5, 14, 20, 3, 11, 20, 7]
MAX_NEW, MAX_PROMPT, SLOTS, S_STAGE = 20, 65, 3, 128
ORDERS = {"forward": list(range(11)), "reversed": list(range(10, -1, -1)), "shuffled": [6, 2, 9, 0, 4, 10, 7, 1, 3, 8, 5]}


def static_batches(model, prompts, **kw):
    """generate() over batches of three of ``prompts`` (the last one filled up with one-row prompts), each padded to S_STAGE rows:
    per request (generated ids of all MAX_NEW steps or up to the batch's end, kept, reason, index)."""
    from magma_amd.sampling import generate
    d = prompts[0].shape[1]
    rows = []
    for i in range(0, len(prompts), 3):
        group = prompts[i:i + 3]
        emb = torch.zeros(3, S_STAGE, d, dtype=BF16, device=model.device)
        lens = [1, 1, 1]
        for r, p in enumerate(group):
            emb[r, : p.shape[0]], lens[r] = p, p.shape[0]
        out = generate(model, emb, lengths=lens, max_steps=MAX_NEW, temperature=0.0, decode=False, **kw)
        out, fin = out if isinstance(out, tuple) else (out, None)
        for r in range(len(group)):
            ids = out[r, lens[r]: lens[r] + MAX_NEW].tolist()
            rows.append((ids,) + ((int(fin.kept[r]), fin.reason[r], fin.index[r]) if fin is not None else (len(ids), "length", -1)))
    return rows


def outcome(ids, limit, eos, seq):
    """(number of tokens kept, reason) of one request's plain greedy ids under the rule."""
    for t in range(limit):
        if ids[t] == eos:
            return t + 1, "eos"
        if seq is not None and t >= 1 and ids[t - 1: t + 1] == seq:
            return t + 1, "stop"
    return limit, "length"


def pick_stops(plain, limits):
    """One eos id that stops at least two requests before their limits and leaves at least four alone, and one two-token stop
    sequence from a request's own ids that stops it early (neither token the eos id)."""
    best = None
    for eos in sorted({t for ids in plain for t in ids}):
        early = [i for i, ids in enumerate(plain) if outcome(ids, limits[i], eos, None) == (outcome(ids, limits[i], eos, None)[0], "eos")
                 and outcome(ids, limits[i], eos, None)[0] < limits[i]]
        if 2 <= len(early) <= len(plain) - 4 and (best is None or len(early) < len(best[1])):
            best = (eos, early)
    assert best is not None, f"no id stops two to seven of the requests early: {plain}"
    eos, early = best
    for i, ids in enumerate(plain):
        if i in early or limits[i] < 4:
            continue
        for t in range(1, limits[i] - 1):
            seq = ids[t - 1: t + 1]
            if eos not in seq and outcome(ids, limits[i], eos, seq) == (t + 1, "stop"):
                return eos, seq
    raise AssertionError(f"no two-token sequence stops a request early: {plain}")


@pytest.fixture(scope="module")
def case(model):  # noqa: F811
    """(prompts, eos id, stop sequence, the reference rows) -- computed once, shared and left unchanged."""
    prompts = embeds(model, LENS, seed=21)
    plain = [r[0] for r in static_batches(model, prompts, eos_token=-7)]
    assert all(len(ids) == MAX_NEW for ids in plain)
    eos, seq = pick_stops(plain, LIMITS)
    ref = []
    for (ids, kept, reason, index), limit in zip(static_batches(model, prompts, eos_token=[eos], stop_sequences=[seq], stop_per_row=True,
                                                                return_finish=True), LIMITS):
        if kept > limit or reason == "length":          # cut at the request's own limit
            kept, reason, index = min(kept, limit), "length", -1
        ref.append((ids[:kept], reason, index))
    # preconditions, on the static runs alone
    assert [(len(r[0]), r[1]) for r in ref] == [outcome(p, n, eos, seq) for p, n in zip(plain, LIMITS)], (ref, plain)
    reasons = [r[1] for r in ref]
    assert reasons.count("eos") >= 2 and "stop" in reasons and reasons.count("length") >= 3, ref
    assert sum(r[1] == "eos" and len(r[0]) < n for r, n in zip(ref, LIMITS)) >= 2, "two requests must stop early at the eos id"
    return prompts, eos, seq, ref


@pytest.fixture
def sessions(monkeypatch):
    """Every SlotSession built during the test."""
    from magma_amd.engine import SlotSession
    made, init = [], SlotSession.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        made.append(self)

    monkeypatch.setattr(SlotSession, "__init__", spy)
    return made


def stream(model, prompts, eos, seq, order=None, **kw):  # noqa: F811
    """generate_stream over the requests in ``order``: {request: StreamResult}, every request exactly once."""
    from magma_amd.sampling import generate_stream
    order = list(range(len(prompts))) if order is None else order
    kw = {**dict(slots=SLOTS, admit_rows=SLOTS, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT, eos_token=[eos],
                 stop_sequences=None if seq is None else [seq], decode=False), **kw}
    got = list(generate_stream(model, [(prompts[i], LIMITS[i]) if i % 2 else (prompts[i][None], LIMITS[i]) for i in order], **kw))
    assert sorted(r.index for r in got) == list(range(len(order))), [r.index for r in got]
    assert all(0 <= r.slot < kw["slots"] and r.tokens.dtype == torch.int64 and r.tokens.device.type == "cpu" for r in got)
    return {order[r.index]: r for r in got}


def rows_of(res):
    return [(res[i].tokens.tolist(), res[i].reason, res[i].reason_index) for i in range(len(res))]


def test_static_ragged_generate_is_permutation_invariant(model):  # noqa: F811
    """The precondition of the reference: a request's ids do not depend on the row of the batch it sits in."""
    from magma_amd.sampling import generate
    prompts = embeds(model, [40, 3, 65], seed=22)
    d = prompts[0].shape[1]

    def run(perm):
        emb = torch.zeros(3, S_STAGE, d, dtype=BF16, device=model.device)
        for r, i in enumerate(perm):
            emb[r, : prompts[i].shape[0]] = prompts[i]
        return generate(model, emb, lengths=[prompts[i].shape[0] for i in perm], max_steps=12, temperature=0.0, eos_token=-7, decode=False)

    a, perm = run([0, 1, 2]), [2, 0, 1]
    b = run(perm)
    for r, i in enumerate(perm):
        n = prompts[i].shape[0]
        assert torch.equal(b[r, n:n + 12], a[i, n:n + 12]), (r, i)
    assert len({tuple(a[i, prompts[i].shape[0]:prompts[i].shape[0] + 12].tolist()) for i in range(3)}) == 3


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("every", [1, 4, 8])
def test_scheduling_changes_nothing(model, case, sessions, every, order):  # noqa: F811
    prompts, eos, seq, ref = case
    res = stream(model, prompts, eos, seq, ORDERS[order], every=every)
    for i, (got, want) in enumerate(zip(rows_of(res), ref)):
        assert got == want, (i, got, want)
    ses, = sessions
    assert ses.steps % every == 0 and all(o is None for o in ses.occ)
    assert len({r.slot for r in res.values()}) == SLOTS


def test_the_ring_wraps(model, case, sessions):  # noqa: F811
    """The requests twice over: the session runs more than two turns of its 32-column ring."""
    from magma_amd.sampling import generate_stream
    prompts, eos, seq, ref = case
    order = ORDERS["shuffled"] + ORDERS["forward"]
    got = list(generate_stream(model, [(prompts[i], LIMITS[i]) for i in order], slots=SLOTS, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT,
                               eos_token=[eos], stop_sequences=[seq], decode=False, every=4))
    assert sorted(r.index for r in got) == list(range(22))
    for r in got:
        assert (r.tokens.tolist(), r.reason, r.reason_index) == ref[order[r.index]], r
    ses, = sessions
    assert ses.Hc == 32 and ses.steps > 2 * ses.Hc, (ses.Hc, ses.steps)


def test_admit_rows_one_is_schedule_invariant(model, case):  # noqa: F811
    """One request per admission prefill (another staging shape than the reference's: its ids are compared among themselves)."""
    prompts, eos, seq, ref = case
    runs = [rows_of(stream(model, prompts, eos, seq, ORDERS[o], every=e, admit_rows=1)) for e, o in ((1, "forward"), (4, "reversed"), (8, "shuffled"))]
    assert runs[0] == runs[1] == runs[2]
    assert [r[1] for r in runs[0]].count("length") >= 3 and all(len(r[0]) <= n for r, n in zip(runs[0], LIMITS))


@pytest.mark.parametrize("sampler", ["reference", "transformers"])
def test_top_k_one_sampling_is_greedy(model, case, sampler):  # noqa: F811
    prompts, eos, seq, ref = case
    res = stream(model, prompts, eos, seq, every=4, temperature=0.7, top_k=1, sampler=sampler, seed=5)
    assert rows_of(res) == ref


def test_sampled_draws_never_share_a_counter(model, case, monkeypatch):  # noqa: F811
    """A sampled session: the (counter word, row) pairs its draws were made under, read from the device at every admission and
    every step, are unique and are what SlotSession.draw_counters states for the schedule the session ran."""
    from magma_amd.engine import SlotSession
    prompts, eos, seq, ref = case
    admit, step, seen, schedule = SlotSession._admit, SlotSession._step, [], []

    def admit_spy(self, batch, slots):
        admit(self, batch, slots)
        seen.extend((int(self.admit_state[0]) & 0xffffffff, j) for j in range(self.n_admit))
        schedule.append(("admit", self.n_admit))

    def step_spy(self):
        seen.extend((int(self.cache.sample_state[0]) & 0xffffffff, b) for b in range(self.B))
        schedule.append(("step", self.B))
        step(self)

    monkeypatch.setattr(SlotSession, "_admit", admit_spy)
    monkeypatch.setattr(SlotSession, "_step", step_spy)
    for admit_rows in (SLOTS, 1):
        seen.clear(), schedule.clear()
        res = stream(model, prompts, eos, seq, every=2, admit_rows=admit_rows, temperature=0.9, top_k=40, seed=7)
        assert all(1 <= len(r.tokens) <= LIMITS[i] for i, r in res.items())
        assert len(set(seen)) == len(seen) > 50 and seen == SlotSession.draw_counters(schedule)
    again = stream(model, prompts, eos, seq, every=2, admit_rows=1, temperature=0.9, top_k=40, seed=7)
    assert rows_of(again) == rows_of(res)                                    # the same seed and schedule: the same draws
    assert rows_of(again) != ref                                             # and they are draws, not the greedy ids


def test_poisoned_idle_memory_changes_nothing(model, case, monkeypatch):  # noqa: F811
    """Between rounds: NaN into the K / V of idle slots, of every position at or past a live row's write position, and of the
    whole staging cache."""
    from magma_amd.engine import SlotSession
    prompts, eos, seq, ref = case
    harvest, rounds = SlotSession._harvest, []

    def poisoned(self):
        out = harvest(self)
        for b, o in enumerate(self.occ):
            at = 0 if o is None else o[2] + (self.steps - o[4])         # an open row's write position (a finished one's lies below)
            self.cache.k[:, b, :, at:] = float("nan")
            self.cache.v[:, b, :, at:] = float("nan")
        self.stage.k.fill_(float("nan"))
        self.stage.v.fill_(float("nan"))
        rounds.append(sum(o is None for o in self.occ))
        return out

    monkeypatch.setattr(SlotSession, "_harvest", poisoned)
    res = stream(model, prompts, eos, seq, ORDERS["shuffled"], every=4)
    assert rows_of(res) == ref
    assert len(rounds) > 5 and max(rounds) >= 1


@pytest.mark.parametrize("switch", ["MAGMA_DECODE_W8", "MAGMA_DECODE_PACK"])
def test_quantised_and_unpacked_steps_are_schedule_invariant(dev, monkeypatch, switch):
    from test_beam_search_gpu import _model
    w8 = switch == "MAGMA_DECODE_W8"
    monkeypatch.setenv(switch, "1" if w8 else "0")
    m = _model(dev, **(dict(n_head=4, mlp_factor=1) if w8 else {}))
    assert m.lm.engine.decode_w8 == w8 and m.lm.engine.decode_pack == w8
    prompts = embeds(m, LENS, seed=23)
    a = rows_of(stream(m, prompts, m.eos_token, None, ORDERS["forward"], every=1))
    b = rows_of(stream(m, prompts, m.eos_token, None, ORDERS["shuffled"], every=8))
    assert a == b and all(1 <= len(r[0]) <= n for r, n in zip(a, LIMITS))


def test_two_sessions_and_plain_calls_interleaved(dev, model, case):  # noqa: F811
    """Two sessions pulled alternately on one engine, plain generate() calls between them: nobody disturbs anybody, and the cache
    pool holds what the plain calls alone leave in it."""
    from magma_amd.sampling import generate, generate_stream
    prompts, eos, seq, ref = case
    eng = model.lm.engine
    plain_in = embeds(model, [9, 30], seed=24)

    def plain():
        return generate(model, plain_in, max_steps=6, temperature=0.0, eos_token=-7, decode=False)

    want_plain = plain()
    pool = dict(eng._cache_pool)
    kw = dict(slots=SLOTS, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT, eos_token=[eos], stop_sequences=[seq], decode=False)
    its = [generate_stream(model, [(prompts[i], LIMITS[i]) for i in ORDERS["forward"]], every=4, **kw),
           generate_stream(model, [(prompts[i], LIMITS[i]) for i in ORDERS["reversed"]], every=1, **kw)]
    got, live, turn = [{}, {}], [True, True], 0
    while any(live):
        s = turn % 2
        turn += 1
        if live[s]:
            r = next(its[s], None)
            if r is None:
                live[s] = False
            else:
                got[s][(ORDERS["forward"], ORDERS["reversed"])[s][r.index]] = r
        if turn % 3 == 0:
            assert torch.equal(plain(), want_plain)
    assert rows_of(got[0]) == ref and rows_of(got[1]) == ref
    assert {k: id(v) for k, v in eng._cache_pool.items()} == {k: id(v) for k, v in pool.items()}
    assert torch.equal(plain(), want_plain)


def test_errors(model, case):  # noqa: F811
    from magma_amd.sampling import generate_stream
    prompts, eos, seq, ref = case
    d = prompts[0].shape[1]
    kw = dict(slots=SLOTS, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT, eos_token=[eos], decode=False)
    long = torch.zeros(MAX_PROMPT + 1, d, dtype=BF16, device=model.device)
    it = generate_stream(model, [(prompts[i], LIMITS[i]) for i in (3, 1, 0, 5)] + [long, prompts[2]], every=2, stop_sequences=[seq], **kw)
    got = []
    with pytest.raises(ValueError, match="request 4"):
        for r in it:
            got.append(r)
    # nothing in front of the failing request is lost: the rows in flight and the request pulled just before it finish first
    assert sorted(r.index for r in got) == [0, 1, 2, 3]
    for r in got:
        assert (r.tokens.tolist(), r.reason, r.reason_index) == ref[(3, 1, 0, 5)[r.index]], r
    assert next(it, None) is None
    assert rows_of(stream(model, prompts, eos, seq, every=8)) == ref             # the engine is as usable as before
    with pytest.raises(ValueError, match="slots"):
        generate_stream(model, prompts, **{**kw, "slots": 17})
    with pytest.raises(ValueError, match="max_position_embeddings"):
        generate_stream(model, prompts, **{**kw, "max_prompt": 250})
    for bad in [dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=2), dict(suppress_tokens=[1]),
                dict(return_logprobs=True), dict(constraint=[[1, 2]]), dict(guidance_scale=2.0), dict(num_beams=2), dict(penalty_alpha=0.6),
                dict(past_key_values=object())]:
        with pytest.raises(NotImplementedError, match="not combined with generate_stream yet"):
            model.generate_stream(prompts, **kw, **bad)
    res = list(model.generate_stream([prompts[1]], **{**kw, "max_new_tokens": 2}, stop_sequences=[seq]))    # an item without a limit
    assert len(res) == 1 and (res[0].tokens.tolist(), res[0].reason, res[0].reason_index) == ref[1]
