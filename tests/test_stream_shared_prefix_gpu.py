"""A SHARED session prefix on the engine (DESIGN.md "Shared session prefix"): generate_stream(prefix=..., share_prefix=True) on the
reduced model of tests/test_stream_gpu.py, with its eleven requests and limits.  The reference is the existing path,
share_prefix=False: ids agree with it by test_continue_generate_gpu.agree's rule (both paths add in different orders), reasons and
indices wherever the ids do.  Among themselves the shared runs are EXACT: the chunking of the prefix depends on P alone, so a
request's tokens, reason and index do not depend on the order of the requests, ``every``, the number of slots or the form of the
prefix.  The live cache holds the rows' own positions only, the given cache is only read, NaN in everything a live row must not read
changes nothing, every launch path of the token step (GEMV co-launch, stand-alone attention, W8A16, unpacked weights) takes the
shared launches, and a shared session, an unshared one and plain generate() calls on one engine do not disturb each other."""
import pytest
import torch

from test_continue_generate_gpu import agree, embeds, model, oracle  # noqa: F401  (fixtures)
from test_stream_gpu import LENS, LIMITS, MAX_NEW, MAX_PROMPT, ORDERS, S_STAGE, SLOTS, rows_of, sessions, stream  # noqa: F401
from test_stream_prefix_gpu import cases, same, snapshot  # noqa: F401  (cases: a fixture)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
CHUNK = 64                  # ops.PREFIX_CHUNK
AGREE_SHARE = 0.3           # of all generated ids compared with the existing path before a tie (the sibling test's share)


def ceil64(n):
    return -(-n // 64) * 64


def compared_before_a_tie(model, convs, got, ref, what):  # noqa: F811
    """agree (its rule and constants) on every row, and the number of ids compared equal before the first difference."""
    agree(model, convs, got, ref, what)
    n = 0
    for g, r in zip(got, ref):
        same_ids = [x == y for x, y in zip(g, r)]
        n += same_ids.index(False) if False in same_ids else len(same_ids)
    return n


@pytest.mark.parametrize("P", [1, 37, 64, CHUNK + 1])
def test_ids_agree_with_the_existing_path(model, cases, sessions, P):  # noqa: F811
    from magma_amd import ops
    assert ops.PREFIX_CHUNK == CHUNK
    prefix, cache, prompts, eos, seq, _, _ = cases(P)
    want = rows_of(stream(model, prompts, eos, seq, ORDERS["shuffled"], every=4, prefix=prefix))
    got = rows_of(stream(model, prompts, eos, seq, ORDERS["shuffled"], every=4, prefix=prefix, share_prefix=True))
    unshared, shared = sessions
    assert not unshared.shared and unshared.cache.prefix_P == 0 and unshared.st.shared is None
    assert shared.shared and shared.cache.prefix_P == P and shared.st.shared[0] == P
    convs = [torch.cat([prefix, p], 0) for p in prompts]
    n = compared_before_a_tie(model, convs, [g[0] for g in got], [w[0] for w in want], f"shared against unshared, P = {P}")
    total = sum(len(w[0]) for w in want)
    print(f"P = {P}: {n} of {total} ids compared before a tie ({n / total:.0%})")
    assert n >= AGREE_SHARE * total, (n, total)
    for i, (g, w) in enumerate(zip(got, want)):
        if g[0] == w[0]:
            assert g[1:] == w[1:], (P, i, g, w)


@pytest.mark.parametrize("slots", [3, 5])
def test_scheduling_slots_and_the_form_of_the_prefix_change_nothing(model, cases, sessions, slots):  # noqa: F811
    P = CHUNK + 1
    prefix, cache, prompts, eos, seq, _, _ = cases(P)
    before = snapshot(cache)
    first = rows_of(stream(model, prompts, eos, seq, ORDERS["forward"], every=1, slots=3, admit_rows=3, prefix=prefix, share_prefix=True))
    reasons = [r[1] for r in first]
    assert "length" in reasons and len({tuple(r[0]) for r in first}) > 3, first
    for every in (1, 8):
        for order, given in (("forward", cache), ("shuffled", prefix), ("shuffled", cache), ("reversed", prefix[None])):
            res = stream(model, prompts, eos, seq, ORDERS[order], every=every, slots=slots, admit_rows=3, prefix=given, share_prefix=True)
            for i, (got, want) in enumerate(zip(rows_of(res), first)):
                assert got == want, (slots, every, order, type(given).__name__, i, got, want)
            assert len({r.slot for r in res.values()}) == slots
    assert same(snapshot(cache), before)
    for ses in sessions:
        assert ses.shared and ses.P == P and all(o is None for o in ses.occ)
        # the live cache holds the rows' own positions only; the staging cache is what it was
        assert ses.cache.Smax == ceil64(MAX_PROMPT + MAX_NEW) and ses.stage.Smax == P + S_STAGE
        assert tuple(ses.cache.prefix_k.shape) == (len(ses.cache), 1, ses.cache.k.shape[2], P, 256) == tuple(ses.cache.prefix_v.shape)
        assert tuple(ses.st.shared[1].shape) == (ses.B, ses.cache.k.shape[2], 2, 264)
        assert torch.equal(ses.cache.prefix_k.view(torch.int16), cache.k[:, :, :, :P].view(torch.int16))
        assert torch.equal(ses.cache.prefix_v.view(torch.int16), cache.v[:, :, :, :P].view(torch.int16))


def test_the_ring_wraps_and_the_given_cache_is_only_read(model, cases, sessions):  # noqa: F811
    """The requests twice over: more than two turns of the 32-column ring, every slot re-admitted several times."""
    from magma_amd.sampling import generate_stream
    P = 37
    prefix, cache, prompts, eos, seq, _, _ = cases(P)
    ref = rows_of(stream(model, prompts, eos, seq, every=8, prefix=prefix, share_prefix=True))
    before = snapshot(cache)
    order = ORDERS["shuffled"] + ORDERS["forward"]
    got = list(generate_stream(model, [(prompts[i], LIMITS[i]) for i in order], slots=SLOTS, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT,
                               eos_token=[eos], stop_sequences=[seq], decode=False, every=4, prefix=cache, share_prefix=True))
    assert sorted(r.index for r in got) == list(range(22))
    for r in got:
        assert (r.tokens.tolist(), r.reason, r.reason_index) == ref[order[r.index]], r
    ses = sessions[-1]
    assert ses.Hc == 32 and ses.steps > 2 * ses.Hc, (ses.Hc, ses.steps)
    assert min(sum(r.slot == b for r in got) for b in range(SLOTS)) >= 3
    assert same(snapshot(cache), before)
    assert ses.cache.Smax == ceil64(MAX_PROMPT + MAX_NEW)
    assert torch.equal(ses.cache.prefix_k.view(torch.int16), cache.k[:, :, :, :P].view(torch.int16))
    assert cache.expand(2).rows_pos().tolist() == [P, P]          # the cache is still the caller's to expand and continue


def test_poisoned_idle_memory_changes_nothing(model, cases, monkeypatch):  # noqa: F811
    """Between rounds: NaN into every byte a live row must not read -- every own position at or past a live row's write index, all
    of an idle slot, the staging cache outside [0, P), and the whole partials scratch (every step rewrites what it reads)."""
    from magma_amd.engine import SlotSession
    P = CHUNK + 1
    prefix, cache, prompts, eos, seq, _, _ = cases(P)
    ref = rows_of(stream(model, prompts, eos, seq, ORDERS["shuffled"], every=4, prefix=prefix, share_prefix=True))
    harvest, rounds = SlotSession._harvest, []

    def poisoned(self):
        out = harvest(self)
        assert self.P == P and self.shared
        for b, o in enumerate(self.occ):
            at = 0 if o is None else o[2] + (self.steps - o[4])      # an open row's own write index (a finished one's lies below)
            self.cache.k[:, b, :, at:] = float("nan")
            self.cache.v[:, b, :, at:] = float("nan")
        self.stage.k[:, :, :, P:] = float("nan")
        self.stage.v[:, :, :, P:] = float("nan")
        self.st.shared[1].fill_(float("nan"))
        rounds.append(sum(o is None for o in self.occ))
        return out

    monkeypatch.setattr(SlotSession, "_harvest", poisoned)
    res = stream(model, prompts, eos, seq, ORDERS["shuffled"], every=4, prefix=prefix, share_prefix=True)
    assert rows_of(res) == ref
    assert len(rounds) > 5 and max(rounds) >= 1


@pytest.mark.parametrize("path", ["co-launch", "stand-alone", "MAGMA_DECODE_W8", "MAGMA_DECODE_PACK"])
def test_every_launch_path_takes_the_shared_launches(dev, monkeypatch, sessions, path):
    """One configuration per launch path of the token step: a block kind that co-launches the attention with a GEMV, an
    attention-only-adapter model (the generic block: the attention launch stands alone), W8A16, and unpacked bf16 weights."""
    from magma_amd import ops
    from test_beam_search_gpu import _model
    kw = {}
    if path == "stand-alone":
        kw = dict(mlp_factor=None, attn_factor=8)
    elif path == "MAGMA_DECODE_W8":
        monkeypatch.setenv(path, "1")
        kw = dict(n_head=4, mlp_factor=1)
    elif path == "MAGMA_DECODE_PACK":
        monkeypatch.setenv(path, "0")
    m = _model(dev, **kw)
    eng = m.lm.engine
    assert eng.decode_w8 == (path == "MAGMA_DECODE_W8") and eng.decode_pack == (path != "MAGMA_DECODE_PACK")
    seen = {"prefix": 0, "gemv": 0, "alone": 0, "unshared": 0}
    for name, key in (("attn_decode_prefix", "prefix"), ("decode_attn_gemv", "gemv"), ("attn_decode_fused", "alone")):
        def spy(*a, _fn=getattr(ops, name), _key=key, **k):
            seen[_key if _key == "prefix" or k.get("shared") is not None else "unshared"] += 1
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    P = CHUNK + 1
    prompts, prefix = embeds(m, LENS, seed=23), embeds(m, [P], seed=25)[0]
    # an eos id of no use to the model: the rows run through token steps, to their limits or near them
    a = rows_of(stream(m, prompts, 3, None, ORDERS["forward"], every=1, prefix=prefix, share_prefix=True))
    assert seen["unshared"] == 0 and seen["prefix"] >= 1, seen
    assert (seen["alone"], seen["gemv"]) == ((seen["prefix"], 0) if path == "stand-alone" else (0, seen["prefix"])), (path, seen)
    kinds = set(sessions[0].st.kinds)
    assert len(kinds) == 1 and ("generic" in kinds) == (path == "stand-alone"), kinds
    b = rows_of(stream(m, prompts, 3, None, ORDERS["shuffled"], every=8, prefix=m.cache_prompt(prefix[None]), share_prefix=True))
    assert a == b and all(1 <= len(r[0]) <= n for r, n in zip(a, LIMITS)) and sum(len(r[0]) for r in a) > 2 * len(LIMITS)
    seen["unshared"] = 0
    u = rows_of(stream(m, prompts, 3, None, ORDERS["forward"], every=1, prefix=prefix))
    assert seen["unshared"] >= 1
    if path != "MAGMA_DECODE_W8":       # agree() judges ties on the bf16 forward: the quantised step is compared among itself above
        agree(m, [torch.cat([prefix, p], 0) for p in prompts], [r[0] for r in a], [r[0] for r in u], f"{path}: shared against unshared")


def test_a_shared_session_an_unshared_one_and_plain_calls_interleaved(dev, model, cases):  # noqa: F811
    from magma_amd.sampling import generate, generate_stream
    P = 37
    prefix, cache, prompts, eos, seq, _, _ = cases(P)
    want = [rows_of(stream(model, prompts, eos, seq, every=4, prefix=prefix, share_prefix=True)),
            rows_of(stream(model, prompts, eos, seq, every=1, prefix=cache))]
    eng = model.lm.engine
    plain_in = embeds(model, [9, 30], seed=24)

    def plain():
        return generate(model, plain_in, max_steps=6, temperature=0.0, eos_token=-7, decode=False)

    want_plain = plain()
    pool = dict(eng._cache_pool)
    kw = dict(slots=SLOTS, max_new_tokens=MAX_NEW, max_prompt=MAX_PROMPT, decode=False, eos_token=[eos], stop_sequences=[seq])
    orders = (ORDERS["forward"], ORDERS["reversed"])
    its = [generate_stream(model, [(prompts[i], LIMITS[i]) for i in orders[0]], every=4, prefix=cache, share_prefix=True, **kw),
           generate_stream(model, [(prompts[i], LIMITS[i]) for i in orders[1]], every=1, prefix=prefix, share_prefix=False, **kw)]
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
    assert rows_of(got[0]) == want[0] and rows_of(got[1]) == want[1]
    assert {k: id(v) for k, v in eng._cache_pool.items()} == {k: id(v) for k, v in pool.items()}
    assert torch.equal(plain(), want_plain)
    with pytest.raises(ValueError, match="share_prefix=True needs a prefix"):
        generate_stream(model, prompts, share_prefix=True, **kw)
    with pytest.raises(ValueError, match="share_prefix=True needs a prefix"):
        model.generate_stream(prompts, share_prefix=True, **kw)
    with pytest.raises(NotImplementedError, match="not combined with generate_stream yet"):
        model.generate_stream(prompts, prefix=cache, share_prefix=True, past_key_values=cache, **kw)
