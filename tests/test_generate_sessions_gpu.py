"""State that survives between generate() calls (DESIGN.md "KV cache": the reuse pool): a call on a pooled KV cache must give
what the same call gives on a fresh one.

Two reduced models with the same parameters.  The SESSION model runs calls in some order on one engine whose pool is never
touched; the REFERENCE model has its pool cleared before every call, so each call allocates its cache, plans its decode state
and captures its graphs from nothing.  Both run the same kernels with the same launch arguments: every comparison is exact
(ids, beam scores, Finish), and every reference call is run twice and must repeat itself.  The fresh-cache path itself is
compared with the fp32 oracle and the host rules by the feature tests; here only reuse is under test.

  * the scripted session (tests/session_cases.py) in order, reversed and shuffled, and under pool bounds 1, 2 and 4;
  * leftovers of the previous call overwritten between calls (a large finite value, then NaN) in every pooled cache;
  * the pool's policy: least recently used goes first, MAGMA_CACHE_POOL = 0 pools nothing, a negative value is refused, an
    evicted cache is freed."""
import gc
import random
import weakref

import pytest
import torch

import session_cases as SC

pytestmark = pytest.mark.gpu


def _model(dev):
    """The reduced model with the oracle's seeded weights, adapters scaled up so that rows differ (test_continue_generate_gpu.py)."""
    from magma_amd.testing import build_reduced_magma
    from oracle.model import OracleConfig, init_params
    cfg = OracleConfig.tiny(mlp_adapter_hidden=128, attn_adapter_hidden=0)
    params = init_params(cfg, seed=11)
    for k in params:
        if ".adapter." in k:
            params[k] = params[k] * 20
    m = build_reduced_magma(dev)
    _, unexpected = m.load_checkpoint_state(params)
    assert not unexpected, unexpected
    m.eval()
    return m


class Reference:
    """Results of calls on a cache that has served nothing else, computed once per unit and kept."""

    def __init__(self, model):
        self.model, self.done = model, {}

    def _unit(self, unit):
        res, past = [], None
        for call in unit:
            self.model.lm.engine._cache_pool.clear()
            r, past = SC.run_call(self.model, call, past)
            res.append(r)
        return res

    def unit(self, unit):
        if unit[0].name not in self.done:
            a, b = self._unit(unit), self._unit(unit)
            for call, x, y in zip(unit, a, b):       # the precondition of an exact comparison
                assert not SC.differences(x, y), f"{call.name} does not repeat itself on a fresh cache: {SC.differences(x, y)}"
                self.done[call.name] = x
        return [self.done[c.name] for c in unit]

    def __getitem__(self, name):
        return self.done[name]

    def probe(self, call):
        return SC.generated(call, self.unit([call])[0])


@pytest.fixture(scope="module")
def ref(dev):
    return Reference(_model(dev))


@pytest.fixture(scope="module")
def script(ref):
    units, pairs = SC.build_script(ref.probe)
    for u in units:
        ref.unit(u)
    return units, pairs


@pytest.fixture(scope="module")
def session_model(dev):
    return _model(dev)


@pytest.fixture
def model(session_model):
    """The session model with a new engine: an empty pool, nothing captured."""
    session_model.lm.invalidate_packed()
    yield session_model
    session_model.lm.invalidate_packed()


def run_session(model, units, ref, pool_max=None, between=None, after=None):
    """The units in order on the model's engine.  After every call: its result is the reference's, the pool is within its
    bound and holds no cache that was handed to a caller.  Returns (results by name, caches returned by name)."""
    eng = model.lm.engine
    if pool_max is not None:
        eng._cache_pool_max = pool_max
    results, returned = {}, {}
    for unit in units:
        want, past = ref.unit(unit), None
        for call, w in zip(unit, want):
            if between is not None:
                between(eng)
            got, new = SC.run_call(model, call, past)
            assert not SC.differences(got, w), f"{call.name} after {list(results)[-3:]}: {SC.differences(got, w)}"
            assert new is None or past is None or new is past, call.name       # a continued cache is advanced in place
            past = new
            if past is not None:
                returned[call.name] = past
            results[call.name] = got
            assert len(eng._cache_pool) <= eng._cache_pool_max, (call.name, list(eng._cache_pool))
            assert not any(c is r for c in eng._cache_pool.values() for r in returned.values()), call.name
            if after is not None:
                after(call, eng, returned)
    return results, returned


def test_the_script_holds_every_pair_and_its_rules_fire(script, ref):
    units, pairs = script
    SC.check_pairs(units, pairs)
    assert len(pairs) == 11 and sum(len(u) for u in units) >= 24
    flat = {c.name: c for u in units for c in u}
    keys = {c.key for c in flat.values() if c.key is not None}
    assert len(keys) > 4 and {k[0] for k in keys} == {1, 2, 4, 8} and {k[1] for k in keys} <= {64, 128}, keys
    assert all(5 <= n <= 40 for c in flat.values() if c.past != "cont" for n in c.lens)
    assert all(6 <= c.steps <= 24 for c in flat.values())
    gen = lambda n: SC.generated(flat[n], ref[n])  # noqa: E731
    # the reference's own results say that the script exercises what it claims to
    assert not SC.differences(ref["s2_seed5"], ref["s2_seed5_again"]) and SC.differences(ref["s2_seed5"], ref["s2_seed6"])
    assert SC.differences(ref["s2_seed5"], ref["s2_other_values"]) and SC.differences(ref["s2_seed5"], ref["s2_transformers_min_p"])
    assert flat["g2_eos1"].kw["eos_token"] in gen("g2_eos1")[0] and flat["g2_eos2"].kw["eos_token"] in gen("g2_eos2")[1]
    ab, cd = flat["p4_suppress_ab"].kw["suppress_tokens"], flat["p4_suppress_cd"].kw["suppress_tokens"]
    assert any(t in row for row in gen("p4_plain") for t in ab) and any(t in row for row in gen("p4_plain") for t in cd)
    assert not any(t in row for row in gen("p4_suppress_ab") for t in ab)
    assert not any(t in row for row in gen("p4_suppress_cd") for t in cd)
    assert SC.differences({"ids": ref["p4_suppress_ab"]["ids"]}, {"ids": ref["p4_suppress_cd"]["ids"]})
    fa, fb = ref["t2_stop_a"]["finish"], ref["t2_stop_b"]["finish"]
    assert "length" not in fa.reason + fb.reason and {"eos", "stop"} <= set(fa.reason + fb.reason), (fa, fb)
    assert SC.differences(ref["t2_stop_a"], ref["t2_stop_b"])
    plain = SC.generated(flat["l1_ends_early"], ref["l1_probe"])[0]
    early, later = (plain.index(flat[n].kw["eos_token"]) for n in ("l1_ends_early", "l1_ends_later"))
    assert early < later < 8 and ref["l1_ends_early"]["ids"].shape[1] == 12 + early + 1
    assert ref["l1_ends_later"]["ids"].shape[1] == 12 + later + 1 and ref["l1_runs_on"]["ids"].shape[1] == 12 + 10
    assert ref["b4_k4_scores"]["scores"].shape == (1,) and ref["b4_k2"]["ids"].shape[0] == 2
    ec = flat["c4_returns_cache"].kw["eos_token"]
    rows = gen("c4_returns_cache")
    assert ec in rows[0] and any(ec not in r for r in rows[1:]), rows           # a row cut back at eos and rows left pending


def test_session_in_order(model, script, ref):
    units, pairs = script
    seen = {}

    def after(call, eng, returned):
        seen[call.name] = dict(eng._cache_pool)

    results, returned = run_session(model, units, ref, after=after)
    eng = model.lm.engine
    assert eng._cache_pool_max == 4
    assert not SC.differences(results["s2_seed5"], results["s2_seed5_again"])
    # the ragged and the uniform cache of one (B, Smax) are two entries, and the ragged call got its own back
    r8, u8 = (8, 64, True), (8, 64, False)
    assert seen["u8_uniform"][r8] is seen["r8_ragged"][r8] and seen["r8_ragged_again"][r8] is seen["r8_ragged"][r8]
    assert seen["r8_ragged_again"][u8] is seen["u8_uniform"][u8]
    # a returned cache left the pool: the next call of its shape got another object
    k2 = (2, 64, True)
    assert k2 not in seen["k2_returns_cache"] and seen["k2_same_shape"][k2] is not returned["k2_returns_cache"]
    assert returned["k2_continued"] is returned["k2_returns_cache"]
    # the cache that served beam search, then a greedy call, went to the caller without its beam buffers
    c4 = (4, 64, False)
    assert returned["c4_returns_cache"] is seen["b4_k4_rules"][c4] and returned["c4_returns_cache"].beam is None


@pytest.mark.parametrize("order", ["reversed", 20, 21, 22])
def test_session_in_another_order(model, script, ref, order):
    """Reversed, and three fixed shuffles (``order`` is the seed); a call that returns its cache keeps its continuations."""
    units = list(script[0])
    if order == "reversed":
        units.reverse()
    else:
        random.Random(order).shuffle(units)
    assert [u[0].name for u in units] != [u[0].name for u in script[0]]
    run_session(model, units, ref)


@pytest.mark.parametrize("bound", [1, 2, 4])
def test_pool_bound(model, script, ref, bound):
    run_session(model, script[0], ref, pool_max=bound)
    assert 1 <= len(model.lm.engine._cache_pool) <= bound


# ---- leftovers of the previous call ----------------------------------------------------------------------------------------

def _overwrite(eng, real, token):
    """Everything in every pooled cache that the next call has no right to read: every K / V slot, the token history, the
    decode state's tensors (scratch, logits, token, ids), the beam buffers, the finish record -- and the suppress ids and the
    stop table WHOLLY, with their host copies reset, so that the next call that uses one must write it again (of the two ways
    to treat these two buffers, this is the one taken here)."""
    def fill(t):
        t.fill_(real if t.is_floating_point() else token)

    for cache in eng._cache_pool.values():
        for t in (cache.k, cache.v, cache.history):
            fill(t)
        for holder in (cache.decode_state, cache.beam):
            for t in vars(holder).values() if holder is not None else ():
                if torch.is_tensor(t):
                    fill(t)
        for t in (cache.finish, cache.suppress, cache.stop_table):
            if t is not None:
                fill(t)
        cache.suppress_ids, cache.stop_held = (), None


def _mixed_session(ref):
    """greedy ragged, sampled, processors + per-row stopping, beam search: four calls on the ragged and the uniform cache of 4
    rows, twice over, so that every call also lands on a cache that the others have used."""
    r = ref.probe(SC.Call("m4_probe", [8] * 4, 10, prompt=33))
    calls = [SC.Call("m4_greedy_ragged", [6, 11, 8, 14], 9, ragged=True, prompt=31, eos_token=r[0][1]),
             SC.Call("m4_sampled", [9] * 4, 8, prompt=32, temperature=0.9, top_k=30, top_p=0.9, seed=7),
             SC.Call("m4_rules_stop", [8] * 4, 10, prompt=33, eos_token=[r[0][2], r[1][4]], stop_sequences=[r[2][3:5]],
                     repetition_penalty=1.2, suppress_tokens=[r[3][0], r[3][1]], return_finish=True),
             SC.Call("m4_beam", [7, 7], 8, prompt=34, num_beams=2, return_scores=True, eos_token=r[0][1]),
             SC.Call("m4_rules_stop_ragged", [6, 11, 8, 14], 9, ragged=True, prompt=31, eos_token=[r[0][2]], stop_sequences=[r[2][3:5]],
                     no_repeat_ngram_size=2, suppress_tokens=[r[3][0]], return_finish=True)]
    return [[c] for c in calls]


@pytest.mark.parametrize("kind", ["finite", "nan"])
def test_leftovers_of_the_previous_call_are_never_read(model, ref, kind):
    """``finite``: bf16 6e4 and the id V - 1 -- a difference means that a kernel or the bookkeeping consumed a stale value.
    ``nan``: NaN and -1 -- as ``finite``, and a masked-out K / V slot must not reach the output through 0 x NaN either."""
    V = model.lm.engine.V
    real, token = (6e4, V - 1) if kind == "finite" else (float("nan"), -1)
    units = _mixed_session(ref)
    run_session(model, units + units, ref, between=lambda eng: _overwrite(eng, real, token))
    assert len(model.lm.engine._cache_pool) == 2


# ---- the pool's policy -----------------------------------------------------------------------------------------------------

def _plain(name, B, ragged=False, seed=40):
    lens = [7 + 2 * b for b in range(B)] if ragged else [9] * B
    return [SC.Call(name, lens, 6, ragged=ragged, prompt=seed + B)]


def test_least_recently_used_goes_first(model, ref):
    A, B, C, D, E = (_plain("lru_a", 1), _plain("lru_b", 2), _plain("lru_c", 4), _plain("lru_d", 8), _plain("lru_e", 2, ragged=True))
    eng = model.lm.engine
    assert eng._cache_pool_max == 4
    run_session(model, [A, B, C, D], ref)
    first_b = eng._cache_pool[B[0].key]
    run_session(model, [A, E], ref)
    assert list(eng._cache_pool) == [C[0].key, D[0].key, A[0].key, E[0].key]      # iteration order = recency order
    run_session(model, [B], ref)                                                 # re-allocated, and C went
    assert list(eng._cache_pool) == [D[0].key, A[0].key, E[0].key, B[0].key] and eng._cache_pool[B[0].key] is not first_b


def test_cache_pool_0_pools_nothing(session_model, ref, script, monkeypatch):
    lm = session_model.lm
    monkeypatch.setenv("MAGMA_CACHE_POOL", "0")
    lm.invalidate_packed()
    try:
        eng = lm.engine
        assert eng._cache_pool_max == 0
        made, prefill = [], eng.prefill

        def recording(*a, **kw):
            out = prefill(*a, **kw)
            made.append(out[1])
            return out

        monkeypatch.setattr(eng, "prefill", recording)
        units = [_plain("lru_b", 2), _plain("lru_b", 2), _plain("lru_e", 2, ragged=True)] + \
            [u for u in script[0] if u[0].name in ("b4_k4_rules", "c4_returns_cache", "s2_seed5")] + [_plain("lru_b", 2)]
        run_session(session_model, units, ref)
        assert len(eng._cache_pool) == 0
        assert len(made) == len(units) and len({id(c) for c in made}) == len(made)    # a new cache for every call
    finally:
        monkeypatch.undo()
        lm.invalidate_packed()


def test_negative_cache_pool_is_refused(session_model, monkeypatch):
    lm = session_model.lm
    monkeypatch.setenv("MAGMA_CACHE_POOL", "-1")
    lm.invalidate_packed()
    try:
        with pytest.raises(ValueError, match="MAGMA_CACHE_POOL"):
            lm.engine
    finally:
        monkeypatch.undo()
        lm.invalidate_packed()


def test_an_evicted_cache_is_freed(model, ref, script):
    """The pool held the only reference: nothing captured on the cache (greedy and beam steps, the beam buffers) keeps its K / V
    alive once it is evicted."""
    eng = model.lm.engine
    beam = [u for u in script[0] if u[0].name in ("b4_k4_scores", "b4_k2")]
    run_session(model, [_plain("lru_c", 4)] + beam, ref, pool_max=1)
    (cache,) = eng._cache_pool.values()
    assert cache.decode_state.graphs and cache.beam is not None
    k, stage = weakref.ref(cache.k), weakref.ref(cache.beam.kstage)
    del cache
    run_session(model, [_plain("lru_a", 1)], ref)
    assert list(eng._cache_pool) == [(1, 64, False)]
    gc.collect()
    assert k() is None and stage() is None
