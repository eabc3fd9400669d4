"""Per-request sampling on the engine (DESIGN.md "Per-request sampling"), on the reduced model of
tests/test_continue_generate_gpu.py: generate() with per-row ``temperature / top_k / top_p / min_p / seed`` and
generate_stream(per_request=True).

The rule is a construction: a row's j-th token is drawn from the Philox stream keyed by ITS seed at counter j over ITS logits
filtered by ITS settings -- the key and counter of the one-row call.  So every comparison is equality of token lists: a row of a
per-row call against its solo call (under the asserted precondition that the two batch shapes give the same greedy ids, i.e. the
claim is about the draw, not about prefill shapes), a permuted batch against the permutation, a streamed request against the
static per-row call over the same staging shape, whatever the slot, the order, ``every`` and the neighbours are."""
import pytest
import torch

from test_continue_generate_gpu import embeds, model, oracle  # noqa: F401  (fixtures)
from test_stream_gpu import (LENS, LIMITS, MAX_NEW, MAX_PROMPT, ORDERS, S_STAGE, SLOTS, case, rows_of,  # noqa: F401  (case: fixture)
                             sessions)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
STEPS = 12
TEMPS = (0.0, 0.7, 1.1)


def tokens(out, lens, steps=STEPS):
    return [out[b, n: n + steps].tolist() for b, n in enumerate(lens)]


def padded(model, prompts, width=None):  # noqa: F811
    width = width or max(p.shape[0] for p in prompts)
    emb = torch.zeros(len(prompts), width, prompts[0].shape[1], dtype=BF16, device=model.device)
    for r, p in enumerate(prompts):
        emb[r, : p.shape[0]] = p
    return emb, [p.shape[0] for p in prompts]


# ---- static per-row generate ------------------------------------------------------------------------------------------------------
ROWS = dict(temperature=[0.0, 0.7, 1.2], top_k=[0, 40, 5], seed=[3, 4, 5])


@pytest.fixture(scope="module")
def trio(model):  # noqa: F811
    """Three ragged prompts padded to one shape whose greedy ids are the same in the B = 3 call and in the B = 1 calls (asserted:
    the precondition of comparing draws across the two shapes)."""
    from magma_amd.sampling import generate
    prompts = embeds(model, [40, 3, 65], seed=22)
    emb, lens = padded(model, prompts)
    kw = dict(max_steps=STEPS, temperature=0.0, eos_token=-7, decode=False)
    together = tokens(generate(model, emb, lengths=lens, **kw), lens)
    alone = [tokens(generate(model, emb[b:b + 1], lengths=lens[b:b + 1], **kw), lens[b:b + 1])[0] for b in range(3)]
    assert together == alone, "pick other prompts: these decode differently at B = 3 and B = 1 already when greedy"
    return prompts, emb, lens, together


@pytest.mark.parametrize("sampler", ["reference", "transformers"])
def test_rows_equal_their_solo_calls(model, trio, sampler, monkeypatch):  # noqa: F811
    from magma_amd import ops
    from magma_amd.sampling import generate
    prompts, emb, lens, greedy = trio
    calls = []
    for name in ("argmax", "sample", "sample_warp", "sample_rows"):
        monkeypatch.setattr(ops, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(getattr(ops, name), name))
    extra = dict(min_p=[0.0, 0.05, 0.0], top_p=[0.9, 0.95, 0.5]) if sampler == "transformers" else {}
    kw = dict(max_steps=STEPS, eos_token=-7, decode=False, sampler=sampler, eos_check_every=STEPS)
    got = tokens(generate(model, emb, lengths=lens, **ROWS, **extra, **kw), lens)
    assert calls.count("sample_rows") == len(calls) >= 1       # the per-row launch where the session-wide ones stood, none of those
    for b in range(3):
        solo = {k: v[b] for k, v in {**ROWS, **extra}.items()}
        calls.clear()
        want = tokens(generate(model, emb[b:b + 1], lengths=lens[b:b + 1], **solo, **kw), lens[b:b + 1])[0]
        assert got[b] == want, (b, solo, got[b], want)
        assert calls and "sample_rows" not in calls            # the scalar call keeps its own launches
    assert got[0] == greedy[0] and got[1] != greedy[1] and got[2] != greedy[2]     # row 0 is greedy, the others are draws
    again = tokens(generate(model, emb, lengths=lens, **ROWS, **extra, **kw), lens)
    assert again == got
    other = tokens(generate(model, emb, lengths=lens, **{**ROWS, "seed": [3, 4, 6]}, **extra, **kw), lens)
    assert other[:2] == got[:2] and other[2] != got[2]          # another seed for row 2 changes row 2 alone


def test_permuting_the_rows_permutes_the_outputs(model, trio):  # noqa: F811
    from magma_amd.sampling import generate
    prompts, emb, lens, _ = trio
    kw = dict(max_steps=STEPS, eos_token=-7, decode=False)
    base = tokens(generate(model, emb, lengths=lens, **ROWS, **kw), lens)
    for perm in ([2, 0, 1], [1, 2, 0], [0, 2, 1]):
        e, ln = padded(model, [prompts[i] for i in perm], emb.shape[1])
        got = tokens(generate(model, e, lengths=ln, **{k: [v[i] for i in perm] for k, v in ROWS.items()}, **kw), ln)
        assert got == [base[i] for i in perm], perm


def test_rows_with_rules_stopping_and_logprobs_equal_their_solo_calls(model, trio):  # noqa: F811
    """The per-row launch sits where the session-wide one sat: behind the logits processors, in front of the log-probability and
    per-row bookkeeping launches."""
    from magma_amd.sampling import generate
    prompts, emb, lens, greedy = trio
    eos = greedy[1][5]
    kw = dict(max_steps=STEPS, eos_token=[eos], stop_per_row=True, return_finish=True, return_logprobs=True, top_logprobs=2,
              repetition_penalty=1.3, no_repeat_ngram_size=2, decode=False)
    out, fin, lp = generate(model, emb, lengths=lens, **ROWS, **kw)
    n = out.shape[1] - emb.shape[1]
    for b in range(3):
        o1, f1, l1 = generate(model, emb[b:b + 1], lengths=lens[b:b + 1], **{k: v[b] for k, v in ROWS.items()}, **kw)
        kept = int(fin.kept[b])
        assert kept == int(f1.kept[0]) and fin.reason[b] == f1.reason[0] and fin.index[b] == f1.index[0], b
        assert out[b, lens[b]: lens[b] + kept].tolist() == o1[0, lens[b]: lens[b] + kept].tolist(), b
        assert torch.equal(lp.logprobs[b, :kept].cpu(), l1.logprobs[0, :kept].cpu()), b
    assert 1 <= n <= STEPS


def test_n_samples_of_one_cached_prompt(model):  # noqa: F811
    """cache_prompt + expand(4) with four seeds: four different continuations, each the solo continuation with its seed."""
    from magma_amd.sampling import generate
    prefix, q = embeds(model, [37], seed=41)[0], embeds(model, [6], seed=42)[0]
    cache = model.cache_prompt(prefix[None])
    kw = dict(max_steps=STEPS, eos_token=-7, decode=False, temperature=0.9, top_k=40)
    g4 = generate(model, q[None].repeat(4, 1, 1), past_key_values=cache.expand(4), **{**kw, "temperature": 0.0})
    g1 = generate(model, q[None], past_key_values=cache.expand(1), **{**kw, "temperature": 0.0})
    assert all(g4[b, 6:].tolist() == g1[0, 6:].tolist() for b in range(4)), "precondition: the greedy continuation at B = 4 and B = 1"
    seeds = [11, 12, 13, 14]
    got = generate(model, q[None].repeat(4, 1, 1), past_key_values=cache.expand(4), seed=seeds, **kw)
    rows = [got[b, 6: 6 + STEPS].tolist() for b in range(4)]
    for b, sd in enumerate(seeds):
        solo = generate(model, q[None], past_key_values=cache.expand(1), seed=sd, **kw)
        assert rows[b] == solo[0, 6: 6 + STEPS].tolist(), (b, sd)
    assert len({tuple(r) for r in rows}) >= 3
    assert cache.rows_pos().tolist() == [37]


def test_refusals_and_checks(model, trio):  # noqa: F811
    from magma_amd.sampling import generate
    prompts, emb, lens, _ = trio
    kw = dict(max_steps=2, eos_token=-7, decode=False, lengths=lens)
    with pytest.raises(ValueError, match="seed has 2 entries, the batch 3 rows"):
        generate(model, emb, seed=[1, 2], **kw)
    with pytest.raises(ValueError, match="row 1: min_p needs sampler"):
        generate(model, emb, min_p=[0.0, 0.1, 0.0], **kw)
    with pytest.raises(ValueError, match="row 0: min_p applies to sampled selection"):
        generate(model, emb, temperature=[0.0, 0.7, 0.7], min_p=0.1, sampler="transformers", **kw)
    with pytest.raises(ValueError, match="row 2: top_p"):
        generate(model, emb, top_p=[0.9, 0.9, 1.5], **kw)
    with pytest.raises(ValueError, match="row 1: temperature"):
        generate(model, emb, temperature=[0.7, -1.0, 0.7], **kw)
    with pytest.raises(ValueError, match="row 0: top_k"):
        generate(model, emb, top_k=[-1, 0, 0], **kw)
    for bad in (dict(num_beams=2), dict(return_scores=True), dict(penalty_alpha=0.6, top_k=4),
                dict(guidance_scale=2.0, negative_embeddings=emb)):
        with pytest.raises(NotImplementedError, match="per-row sampler settings"):
            generate(model, emb, seed=[1, 2, 3], **{**kw, **bad})


# ---- generate_stream(per_request=True) --------------------------------------------------------------------------------------------
def settings(i, seed=None):
    t = TEMPS[(i + 1) % 3]
    return dict(temperature=t, top_k=40 if t else 0, seed=100 + i if seed is None else seed)


def stream(model, prompts, eos, seq, order=None, seeds=None, **kw):  # noqa: F811
    """generate_stream(per_request=True) over the requests in ``order``: {request: StreamResult}.  A request comes as a
    StreamRequest with its own settings; the session's keywords differ from all of them."""
    from magma_amd.sampling import StreamRequest, generate_stream
    order = list(range(len(prompts))) if order is None else order
    kw = {**dict(slots=SLOTS, admit_rows=SLOTS, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT, eos_token=[eos],
                 stop_sequences=None if seq is None else [seq], decode=False, per_request=True, temperature=0.3, top_k=7, seed=999), **kw}
    items = [StreamRequest(prompts[i] if i % 2 else prompts[i][None], LIMITS[i], **settings(i, (seeds or {}).get(i))) for i in order]
    got = list(generate_stream(model, items, **kw))
    assert sorted(r.index for r in got) == list(range(len(order))), [r.index for r in got]
    return {order[r.index]: r for r in got}


@pytest.fixture(scope="module")
def sampled(model, case):  # noqa: F811
    """The reference rows of the per-request stream: static per-row generate() over batches of three of the same requests, each
    padded to the session's staging shape (the last batch filled up with a greedy one-row prompt), cut at the request's limit."""
    from magma_amd.sampling import generate
    prompts, eos, seq, greedy_ref = case
    ref = []
    for i in range(0, len(prompts), 3):
        group = list(range(i, min(i + 3, len(prompts))))
        emb, lens = padded(model, [prompts[j] for j in group] + [prompts[0][:1]] * (3 - len(group)), S_STAGE)
        rec = [settings(j) for j in group] + [dict(temperature=0.0, top_k=0, seed=0)] * (3 - len(group))
        out, fin = generate(model, emb, lengths=lens, max_steps=MAX_NEW, decode=False, eos_token=[eos], stop_sequences=[seq],
                            stop_per_row=True, return_finish=True, **{k: [r[k] for r in rec] for k in rec[0]})
        for r, j in enumerate(group):
            kept, reason, index = int(fin.kept[r]), fin.reason[r], fin.index[r]
            if kept > LIMITS[j] or reason == "length":
                kept, reason, index = min(kept, LIMITS[j]), "length", -1
            ref.append((out[r, lens[r]: lens[r] + kept].tolist(), reason, index))
    greedy = [j for j in range(len(prompts)) if settings(j)["temperature"] == 0.0]
    assert len(greedy) == 3 and all(ref[j] == greedy_ref[j] for j in greedy)          # the greedy requests: the existing reference
    assert sum(ref[j] != greedy_ref[j] for j in range(len(prompts)) if j not in greedy) >= 4      # the others are draws
    return ref


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("every", [1, 4])
def test_stream_equals_static_per_row_generate(model, case, sampled, sessions, every, order):  # noqa: F811
    prompts, eos, seq, _ = case
    res = stream(model, prompts, eos, seq, ORDERS[order], every=every)
    for i, (got, want) in enumerate(zip(rows_of(res), sampled)):
        assert got == want, (i, got, want)
    ses, = sessions
    assert ses.plan.is_rows and len({r.slot for r in res.values()}) == SLOTS


def test_stream_ring_wraps_and_runs_repeat(model, case, sampled, sessions):  # noqa: F811
    """The requests twice over in one session (the second copy of a request has the first one's seed: the same tokens, from
    another slot, at another global step, after more than two turns of the 32-column ring)."""
    from magma_amd.sampling import StreamRequest, generate_stream
    prompts, eos, seq, _ = case
    order = ORDERS["shuffled"] + ORDERS["forward"]
    items = [StreamRequest(prompts[i], LIMITS[i], **settings(i)) for i in order]
    got = list(generate_stream(model, items, slots=SLOTS, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT, eos_token=[eos],
                               stop_sequences=[seq], decode=False, every=4, per_request=True))
    assert sorted(r.index for r in got) == list(range(22))
    for r in got:
        assert (r.tokens.tolist(), r.reason, r.reason_index) == sampled[order[r.index]], r
    ses, = sessions
    assert ses.Hc == 32 and ses.steps > 2 * ses.Hc


def test_stream_admit_rows_one_is_schedule_invariant(model, case):  # noqa: F811
    """One request per admission prefill (another staging shape than the reference's: compared among themselves)."""
    prompts, eos, seq, _ = case
    runs = [rows_of(stream(model, prompts, eos, seq, ORDERS[o], every=e, admit_rows=1))
            for e, o in ((1, "forward"), (4, "reversed"), (8, "shuffled"))]
    assert runs[0] == runs[1] == runs[2]
    assert all(1 <= len(r[0]) <= n for r, n in zip(runs[0], LIMITS))


def test_another_seed_changes_that_request_alone(model, case, sampled):  # noqa: F811
    prompts, eos, seq, _ = case
    assert settings(3)["temperature"] > 0 and LIMITS[3] == MAX_NEW
    res = rows_of(stream(model, prompts, eos, seq, ORDERS["shuffled"], every=4, seeds={3: 777}))
    assert res[3] != sampled[3]
    assert [r for i, r in enumerate(res) if i != 3] == [r for i, r in enumerate(sampled) if i != 3]


def test_session_keywords_are_the_defaults(model, case, sampled):  # noqa: F811
    """Plain items and None fields take the session's settings and seed; a request's own fields override them."""
    from magma_amd.sampling import StreamRequest, generate_stream
    prompts, eos, seq, _ = case
    s = settings(3)
    items = [(prompts[3], LIMITS[3]), StreamRequest(prompts[3], LIMITS[3]), StreamRequest(prompts[3], LIMITS[3], seed=s["seed"] + 1),
             StreamRequest(prompts[2], LIMITS[2], temperature=0.0, top_k=0)]
    got = {r.index: r for r in generate_stream(model, items, slots=2, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT, eos_token=[eos],
                                               stop_sequences=[seq], decode=False, per_request=True, admit_rows=2, **s)}
    a, b, c, d = (got[i].tokens.tolist() for i in range(4))
    assert a == b and a != c
    with pytest.raises(ValueError, match="request 1: a StreamRequest needs"):
        list(generate_stream(model, [prompts[1], StreamRequest(prompts[2])], slots=2, max_new_tokens=4, max_prompt=MAX_PROMPT,
                             eos_token=[eos], decode=False))


def test_poisoned_idle_memory_changes_nothing(model, case, sampled, monkeypatch):  # noqa: F811
    """Between rounds: NaN into the K / V of idle slots, of every position at or past a live row's write position and of the
    whole staging cache, and all-ones bytes (NaN settings, a negative top_k) into the records of idle slots and the staging table."""
    from magma_amd.engine import SlotSession
    prompts, eos, seq, _ = case
    harvest, rounds = SlotSession._harvest, []

    def poisoned(self):
        out = harvest(self)
        for b, o in enumerate(self.occ):
            at = 0 if o is None else o[2] + (self.steps - o[4])
            self.cache.k[:, b, :, at:] = float("nan")
            self.cache.v[:, b, :, at:] = float("nan")
            if o is None:
                self.cache.sample_rows[b] = 0xFF
        self.stage.k.fill_(float("nan"))
        self.stage.v.fill_(float("nan"))
        self.stage_rows.fill_(0xFF)
        rounds.append(sum(o is None for o in self.occ))
        return out

    monkeypatch.setattr(SlotSession, "_harvest", poisoned)
    res = stream(model, prompts, eos, seq, ORDERS["shuffled"], every=4)
    assert rows_of(res) == sampled
    assert len(rounds) > 5 and max(rounds) >= 1


@pytest.mark.parametrize("share", [False, True])
def test_prefix_sessions_do_not_depend_on_slot_or_order(model, case, share):  # noqa: F811
    prompts, eos, seq, _ = case
    prefix = embeds(model, [37], seed=43)[0]
    a = rows_of(stream(model, prompts, eos, seq, ORDERS["forward"], every=1, prefix=prefix, share_prefix=share))
    b = rows_of(stream(model, prompts, eos, seq, ORDERS["shuffled"], every=4, prefix=prefix, share_prefix=share))
    assert a == b and all(1 <= len(r[0]) <= n for r, n in zip(a, LIMITS))


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
