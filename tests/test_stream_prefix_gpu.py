"""A session prefix on the engine (DESIGN.md "Request streams", session prefix): generate_stream(prefix=...) on the reduced model
of tests/test_stream_gpu.py, with its eleven requests and limits.  Every request's tokens, reason and index equal, exactly, those
of the static continued call -- generate(batches of three, past_key_values=model.cache_prompt(prefix).expand(3)) -- whatever the
prefix length, ``every``, the order of the requests and the form of the prefix (embeddings or a cache) are; they agree with a
fresh prefill of cat([prefix, request]) up to bf16 ties; the given cache is only read and every slot keeps its prefix; NaN in
everything a live row must not read changes nothing; the admission prefill runs over the requests' rows only; the error cases."""
import pytest
import torch

from test_continue_generate_gpu import agree, embeds, model, oracle  # noqa: F401  (fixtures)
from test_stream_gpu import (LENS, LIMITS, MAX_NEW, MAX_PROMPT, ORDERS, S_STAGE, SLOTS, outcome, pick_stops, rows_of, sessions,  # noqa: F401
                             stream)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
PREFIXES = [1, 31, 37, 64]
FRESH_SHARE = 0.3           # of all generated ids compared with a fresh prefill before a tie (test_continue_generate_gpu's share)


def static_continued(model, cache, prompts, **kw):  # noqa: F811
    """generate() over batches of three of ``prompts`` (the last one filled up with one-row prompts), each padded to S_STAGE rows,
    continued from ``cache`` expanded to three rows: per request (generated ids, kept, reason, index), as
    test_stream_gpu.static_batches."""
    from magma_amd.sampling import generate
    d = prompts[0].shape[1]
    rows = []
    for i in range(0, len(prompts), 3):
        group = prompts[i:i + 3]
        emb = torch.zeros(3, S_STAGE, d, dtype=BF16, device=model.device)
        lens = [1, 1, 1]
        for r, p in enumerate(group):
            emb[r, : p.shape[0]], lens[r] = p, p.shape[0]
        out = generate(model, emb, lengths=lens, past_key_values=cache.expand(3), max_steps=MAX_NEW, temperature=0.0, decode=False, **kw)
        out, fin = out if isinstance(out, tuple) else (out, None)
        for r in range(len(group)):
            ids = out[r, lens[r]: lens[r] + MAX_NEW].tolist()
            rows.append((ids,) + ((int(fin.kept[r]), fin.reason[r], fin.index[r]) if fin is not None else (len(ids), "length", -1)))
    return rows


def snapshot(cache):
    """Everything of a cache a session must leave alone, as bit patterns."""
    return (cache.k.view(torch.int16).clone(), cache.v.view(torch.int16).clone(), cache.d_pos.clone(), cache.rows_pos().clone(),
            cache.pos, None if cache.pending is None else cache.pending.clone())


def same(a, b):
    return all((x is None and y is None) or (torch.equal(x, y) if torch.is_tensor(x) else x == y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def cases(model):  # noqa: F811
    """P -> (prefix embeddings, its cache_prompt cache, prompts, eos id, stop sequence, the reference rows, the plain ids):
    computed once per P, shared and left unchanged."""
    memo = {}
    prompts = embeds(model, LENS, seed=21)

    def get(P):
        if P in memo:
            return memo[P]
        prefix = embeds(model, [P], seed=40 + P)[0]
        cache = model.cache_prompt(prefix[None])
        assert cache.B == 1 and cache.rows_pos().tolist() == [P] and cache.pending is None
        plain = [r[0] for r in static_continued(model, cache, prompts, eos_token=-7)]
        assert all(len(ids) == MAX_NEW for ids in plain)
        eos, seq = pick_stops(plain, LIMITS)
        ref = []
        for (ids, kept, reason, index), limit in zip(static_continued(model, cache, prompts, eos_token=[eos], stop_sequences=[seq],
                                                                      stop_per_row=True, return_finish=True), LIMITS):
            if kept > limit or reason == "length":          # cut at the request's own limit
                kept, reason, index = min(kept, limit), "length", -1
            ref.append((ids[:kept], reason, index))
        # preconditions, on the static runs alone
        assert [(len(r[0]), r[1]) for r in ref] == [outcome(p, n, eos, seq) for p, n in zip(plain, LIMITS)], (ref, plain)
        reasons = [r[1] for r in ref]
        assert reasons.count("eos") >= 2 and "stop" in reasons and reasons.count("length") >= 3, ref
        assert sum(r[1] == "eos" and len(r[0]) < n for r, n in zip(ref, LIMITS)) >= 2, "two requests must stop early at the eos id"
        memo[P] = (prefix, cache, prompts, eos, seq, ref, plain)
        return memo[P]

    return get


def test_static_continued_generate_is_permutation_invariant(model):  # noqa: F811
    """The precondition of the reference: behind a shared prefix cache, a request's ids do not depend on the row it sits in."""
    from magma_amd.sampling import generate
    prompts = embeds(model, [40, 3, 65], seed=22)
    cache = model.cache_prompt(embeds(model, [37], seed=77)[0][None])
    d = prompts[0].shape[1]

    def run(perm):
        emb = torch.zeros(3, S_STAGE, d, dtype=BF16, device=model.device)
        for r, i in enumerate(perm):
            emb[r, : prompts[i].shape[0]] = prompts[i]
        return generate(model, emb, lengths=[prompts[i].shape[0] for i in perm], past_key_values=cache.expand(3), max_steps=12,
                        temperature=0.0, eos_token=-7, decode=False)

    a, perm = run([0, 1, 2]), [2, 0, 1]
    b = run(perm)
    for r, i in enumerate(perm):
        n = prompts[i].shape[0]
        assert torch.equal(b[r, n:n + 12], a[i, n:n + 12]), (r, i)
    assert len({tuple(a[i, prompts[i].shape[0]:prompts[i].shape[0] + 12].tolist()) for i in range(3)}) == 3


@pytest.mark.parametrize("every", [1, 8])
@pytest.mark.parametrize("P", PREFIXES)
def test_scheduling_and_the_form_of_the_prefix_change_nothing(model, cases, sessions, P, every):  # noqa: F811
    prefix, cache, prompts, eos, seq, ref, _ = cases(P)
    before = snapshot(cache)
    for order, given in (("forward", prefix), ("shuffled", cache), ("shuffled", prefix[None]), ("forward", cache)):
        res = stream(model, prompts, eos, seq, ORDERS[order], every=every, prefix=given)
        for i, (got, want) in enumerate(zip(rows_of(res), ref)):
            assert got == want, (P, order, type(given).__name__, i, got, want)
        assert len({r.slot for r in res.values()}) == SLOTS
    assert len(sessions) == 4 and same(snapshot(cache), before)
    for ses in sessions:
        assert ses.steps % every == 0 and all(o is None for o in ses.occ) and ses.P == P
        # the admission prefill runs over the requests' own rows: (admit_rows, ceil64(max_prompt)), not ceil64(P + max_prompt)
        assert tuple(ses.stage_in.shape[:2]) == (SLOTS, S_STAGE) and ses.S_stage == S_STAGE == -(-MAX_PROMPT // 64) * 64
        assert ses.stage.Smax == P + S_STAGE and ses.cache.Smax == -(-(P + MAX_PROMPT + MAX_NEW) // 64) * 64
        assert ses.stage.pending is None and ses.stage.d_pos.tolist() == [P] * SLOTS
    assert -(-(64 + MAX_PROMPT) // 64) * 64 != S_STAGE          # at P = 64 the two shapes differ


def test_the_ring_wraps_and_every_slot_keeps_its_prefix(model, cases, sessions):  # noqa: F811
    """The requests twice over: the session runs more than two turns of its 32-column ring and every slot is re-admitted several
    times; afterwards the given cache is bit for bit what it was and positions [0, P) of every slot still hold the prefix."""
    from magma_amd.sampling import generate_stream
    P = 37
    prefix, cache, prompts, eos, seq, ref, _ = cases(P)
    before = snapshot(cache)
    order = ORDERS["shuffled"] + ORDERS["forward"]
    got = list(generate_stream(model, [(prompts[i], LIMITS[i]) for i in order], slots=SLOTS, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT,
                               eos_token=[eos], stop_sequences=[seq], decode=False, every=4, prefix=cache))
    assert sorted(r.index for r in got) == list(range(22))
    for r in got:
        assert (r.tokens.tolist(), r.reason, r.reason_index) == ref[order[r.index]], r
    ses, = sessions
    assert ses.Hc == 32 and ses.steps > 2 * ses.Hc, (ses.Hc, ses.steps)
    assert min(sum(r.slot == b for r in got) for b in range(SLOTS)) >= 3
    assert same(snapshot(cache), before)
    for own in (ses.cache, ses.stage):
        for b in range(own.B):
            assert torch.equal(own.k[:, b, :, :P].view(torch.int16), cache.k[:, 0, :, :P].view(torch.int16)), b
            assert torch.equal(own.v[:, b, :, :P].view(torch.int16), cache.v[:, 0, :, :P].view(torch.int16)), b
    # the cache is still the caller's to expand and continue
    assert cache.expand(2).rows_pos().tolist() == [P, P]


def test_admit_rows_one_is_schedule_invariant(model, cases):  # noqa: F811
    """One request per admission prefill (another staging shape than the reference's: its ids are compared among themselves)."""
    prefix, cache, prompts, eos, seq, ref, _ = cases(31)
    runs = [rows_of(stream(model, prompts, eos, seq, ORDERS[o], every=e, admit_rows=1, prefix=g))
            for e, o, g in ((1, "forward", prefix), (4, "reversed", cache), (8, "shuffled", prefix))]
    assert runs[0] == runs[1] == runs[2]
    assert [r[1] for r in runs[0]].count("length") >= 3 and all(len(r[0]) <= n for r, n in zip(runs[0], LIMITS))


def compared_before_a_tie(model, convs, got, fresh, what):  # noqa: F811
    """test_continue_generate_gpu.agree (its rule and constants) on every row, and the number of ids compared equal before the
    first difference."""
    agree(model, convs, got, fresh, what)
    n = 0
    for g, r in zip(got, fresh):
        same_ids = [x == y for x, y in zip(g, r)]
        n += same_ids.index(False) if False in same_ids else len(same_ids)
    return n


@pytest.mark.parametrize("P", [37, 64])
def test_ids_agree_with_a_fresh_prefill_of_the_concatenation(model, cases, P):  # noqa: F811
    """Against plain generate() on cat([prefix, request_i]): equal up to the first decision whose fresh top-1 / top-2 gap is within
    0.02 x std(logits), and at least 30 % of all generated ids compared before such a tie -- on the static continued path first
    (the precondition), then on the stream."""
    from magma_amd.sampling import generate
    prefix, cache, prompts, eos, seq, ref, plain = cases(P)
    convs = [torch.cat([prefix, p], 0) for p in prompts]
    out = generate(model, convs, max_steps=MAX_NEW, temperature=0.0, eos_token=-7, decode=False)
    fresh = [out[b, c.shape[0]: c.shape[0] + MAX_NEW].tolist() for b, c in enumerate(convs)]
    n_static = compared_before_a_tie(model, convs, plain, fresh, f"static continued, P = {P}")
    total = sum(len(ids) for ids in plain)
    print(f"P = {P}: static continued path: {n_static} of {total} ids compared before a tie ({n_static / total:.0%})")
    assert n_static >= FRESH_SHARE * total, (n_static, total)         # the precondition: the seed leaves enough to compare
    res = rows_of(stream(model, prompts, eos, seq, ORDERS["shuffled"], every=4, prefix=prefix))
    got = [r[0] for r in res]
    n_stream = compared_before_a_tie(model, convs, got, [f[: len(g)] for f, g in zip(fresh, got)], f"stream, P = {P}")
    total = sum(len(g) for g in got)
    print(f"P = {P}: stream: {n_stream} of {total} ids compared before a tie ({n_stream / total:.0%})")
    assert n_stream >= FRESH_SHARE * total, (n_stream, total)


@pytest.mark.parametrize("sampler", ["reference", "transformers"])
def test_top_k_one_sampling_is_greedy(model, cases, sampler):  # noqa: F811
    prefix, cache, prompts, eos, seq, ref, _ = cases(37)
    res = stream(model, prompts, eos, seq, every=4, temperature=0.7, top_k=1, sampler=sampler, seed=5, prefix=cache)
    assert rows_of(res) == ref


def test_poisoned_idle_memory_changes_nothing(model, cases, monkeypatch):  # noqa: F811
    """Between rounds: NaN into every live-cache byte a live row must not read -- every position at or past a live row's write
    position, all of an idle slot outside [0, P) -- and into the staging cache outside [0, P)."""
    from magma_amd.engine import SlotSession
    P = 31
    prefix, cache, prompts, eos, seq, ref, _ = cases(P)
    harvest, rounds = SlotSession._harvest, []

    def poisoned(self):
        out = harvest(self)
        assert self.P == P
        for b, o in enumerate(self.occ):
            at = P if o is None else P + o[2] + (self.steps - o[4])     # an open row's write position (a finished one's lies below)
            self.cache.k[:, b, :, at:] = float("nan")
            self.cache.v[:, b, :, at:] = float("nan")
        self.stage.k[:, :, :, P:] = float("nan")
        self.stage.v[:, :, :, P:] = float("nan")
        rounds.append(sum(o is None for o in self.occ))
        return out

    monkeypatch.setattr(SlotSession, "_harvest", poisoned)
    res = stream(model, prompts, eos, seq, ORDERS["shuffled"], every=4, prefix=prefix)
    assert rows_of(res) == ref
    assert len(rounds) > 5 and max(rounds) >= 1


@pytest.mark.parametrize("switch", ["MAGMA_DECODE_W8", "MAGMA_DECODE_PACK"])
def test_quantised_and_unpacked_steps_are_schedule_invariant(dev, monkeypatch, switch):
    from test_beam_search_gpu import _model
    w8 = switch == "MAGMA_DECODE_W8"
    monkeypatch.setenv(switch, "1" if w8 else "0")
    m = _model(dev, **(dict(n_head=4, mlp_factor=1) if w8 else {}))
    assert m.lm.engine.decode_w8 == w8 and m.lm.engine.decode_pack == w8
    prompts, prefix = embeds(m, LENS, seed=23), embeds(m, [37], seed=25)[0]
    a = rows_of(stream(m, prompts, m.eos_token, None, ORDERS["forward"], every=1, prefix=prefix))
    b = rows_of(stream(m, prompts, m.eos_token, None, ORDERS["shuffled"], every=8, prefix=m.cache_prompt(prefix[None])))
    assert a == b and all(1 <= len(r[0]) <= n for r, n in zip(a, LIMITS))
    # an eos id of no use to the model (it emits its own at once): the rows run through token steps, to their limits or near them
    a = rows_of(stream(m, prompts, 3, None, ORDERS["forward"], every=1, prefix=prefix))
    b = rows_of(stream(m, prompts, 3, None, ORDERS["shuffled"], every=8, prefix=prefix))
    assert a == b and all(1 <= len(r[0]) <= n for r, n in zip(a, LIMITS)) and sum(len(r[0]) for r in a) > 2 * len(LIMITS)


def test_two_sessions_with_different_prefixes_and_plain_calls_interleaved(dev, model, cases):  # noqa: F811
    """Two sessions with different prefixes pulled alternately on one engine, plain generate() calls between them: nobody disturbs
    anybody, and the cache pool holds what the plain calls alone leave in it."""
    from magma_amd.sampling import generate, generate_stream
    a, b = cases(31), cases(64)
    assert [r[0] for r in a[5]] != [r[0] for r in b[5]]                      # the prefixes matter
    eng = model.lm.engine
    plain_in = embeds(model, [9, 30], seed=24)

    def plain():
        return generate(model, plain_in, max_steps=6, temperature=0.0, eos_token=-7, decode=False)

    want_plain = plain()
    pool = dict(eng._cache_pool)
    kw = dict(slots=SLOTS, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT, decode=False)
    orders = (ORDERS["forward"], ORDERS["reversed"])
    its = [generate_stream(model, [(a[2][i], LIMITS[i]) for i in orders[0]], every=4, prefix=a[0], eos_token=[a[3]], stop_sequences=[a[4]], **kw),
           generate_stream(model, [(b[2][i], LIMITS[i]) for i in orders[1]], every=1, prefix=b[1], eos_token=[b[3]], stop_sequences=[b[4]], **kw)]
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
    assert rows_of(got[0]) == a[5] and rows_of(got[1]) == b[5]
    assert {k: id(v) for k, v in eng._cache_pool.items()} == {k: id(v) for k, v in pool.items()}
    assert torch.equal(plain(), want_plain)


def test_errors(model, cases):  # noqa: F811
    from magma_amd.sampling import generate, generate_stream
    P = 37
    prefix, cache, prompts, eos, seq, ref, _ = cases(P)
    d = prompts[0].shape[1]
    kw = dict(slots=SLOTS, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT, eos_token=[eos], decode=False)
    long = torch.zeros(MAX_PROMPT + 1, d, dtype=BF16, device=model.device)
    it = generate_stream(model, [(prompts[i], LIMITS[i]) for i in (3, 1, 0, 5)] + [long, prompts[2]], every=2, stop_sequences=[seq],
                         prefix=cache, **kw)
    got = []
    with pytest.raises(ValueError, match="request 4"):
        for r in it:
            got.append(r)
    # nothing in front of the failing request is lost: the rows in flight and the request pulled just before it finish first
    assert sorted(r.index for r in got) == [0, 1, 2, 3]
    for r in got:
        assert (r.tokens.tolist(), r.reason, r.reason_index) == ref[(3, 1, 0, 5)[r.index]], r
    assert next(it, None) is None
    assert rows_of(stream(model, prompts, eos, seq, every=8, prefix=cache)) == ref              # the engine is as usable as before
    # refused when the call is made
    many = model.cache_prompt(torch.stack([prefix, prefix]))
    with pytest.raises(ValueError, match="holds 2 rows"):
        generate_stream(model, prompts, prefix=many, **kw)
    with pytest.raises(ValueError, match="holds 3 rows"):
        generate_stream(model, prompts, prefix=cache.expand(3), **kw)
    _, turn = generate(model, prefix[None], max_steps=2, temperature=0.0, eos_token=-7, decode=False, return_past_key_values=True)
    assert turn.pending is not None and int(turn.pending[0]) >= 0
    with pytest.raises(ValueError, match="not been fed back"):
        generate_stream(model, prompts, prefix=turn, **kw)
    from test_beam_search_gpu import _model
    other = _model(model.device)
    with pytest.raises(ValueError, match="another engine"):
        generate_stream(model, prompts, prefix=other.cache_prompt(embeds(other, [P], seed=3)[0][None]), **kw)
    with pytest.raises(ValueError, match="prefix"):
        generate_stream(model, prompts, prefix=torch.zeros(5, d + 1, dtype=BF16, device=model.device), **kw)
    n_pos = model.lm.config.max_position_embeddings
    with pytest.raises(ValueError, match="max_position_embeddings"):
        generate_stream(model, prompts, prefix=torch.zeros(n_pos - MAX_PROMPT - MAX_NEW + 1, d, dtype=BF16, device=model.device), **kw)
    with pytest.raises(NotImplementedError, match="not combined with generate_stream yet"):
        model.generate_stream(prompts, prefix=cache, past_key_values=cache, **kw)
    res = list(model.generate_stream([prompts[1]], **{**kw, "max_new_tokens": 2}, stop_sequences=[seq], prefix=prefix))
    assert len(res) == 1 and (res[0].tokens.tolist(), res[0].reason, res[0].reason_index) == ref[1]
