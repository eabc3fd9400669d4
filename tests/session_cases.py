"""The call script of tests/test_generate_sessions_gpu.py: generate() calls of every mode on a handful of KV-cache pool keys,
the adjacent pairs the tests rely on, and the helpers that run one call and compare two results.

A ``Call`` is one generate() call on the reduced model: prompt lengths (``ragged``: passed as per-row tensors, so the call takes
``lengths``), the seed of its inputs (``prompt``), ``max_steps`` and generate()'s keyword arguments (``seed`` among them).
``past``: None, "new" (the call returns its cache) or "cont" (the call continues the cache the previous call of its unit
returned, and returns it again).  The script is a list of UNITS, each a list of calls that stay together in any order of the
script: a call alone, or a call that returns its cache followed by its continuations.

The token ids in the script (eos ids, stop sequences, suppress ids) are taken from probe runs -- the plain greedy ids of the
prompt in question -- so that the rules they arm do fire."""
import torch

BF16 = torch.bfloat16
NEVER = -7              # an eos id that no row emits
N_POS = 256             # build_reduced_magma's max_position_embeddings


class Call:
    def __init__(self, name, lens, steps, *, ragged=False, prompt=0, past=None, **kw):
        assert ragged or len(set(lens)) == 1, name
        assert past in (None, "new", "cont"), name
        self.name, self.lens, self.steps, self.ragged = name, list(lens), steps, ragged
        self.prompt, self.past, self.kw = prompt, past, kw

    @property
    def beams(self):
        return self.kw.get("num_beams", 1)

    @property
    def key(self):
        """The pool key LMEngine.prefill files this call's cache under (None: a continuation, which takes no pooled cache)."""
        if self.past == "cont":
            return None
        smax = min(N_POS, -(-(max(self.lens) + self.steps) // 64) * 64)
        return (len(self.lens) * self.beams, smax, self.ragged)

    def __repr__(self):
        return f"Call({self.name})"


def inputs(model, call):
    """The call's inputs: (B, S, d) for a uniform call, a list of (s_b, d) rows for a ragged one."""
    g = torch.Generator().manual_seed(1000 + call.prompt)
    d = model.lm.config.hidden_size
    rows = [(torch.randn(n, d, generator=g) * 0.5).to(BF16).to(model.device) for n in call.lens]
    return rows if call.ragged else torch.stack(rows, 0)


def run_call(model, call, past=None):
    """One generate() call -> (dict(ids[, scores][, finish]), the cache it returned or None)."""
    from magma_amd.sampling import generate
    kw = dict(max_steps=call.steps, temperature=0.0, eos_token=NEVER, decode=False)
    kw.update(call.kw)
    if call.past is not None:
        kw["return_past_key_values"] = True
    if call.past == "cont":
        assert past is not None, f"{call.name}: nothing to continue"
        kw["past_key_values"] = past
    out = generate(model, inputs(model, call), **kw)
    out = list(out) if isinstance(out, tuple) else [out]
    res = {"ids": out.pop(0)}
    new_past = out.pop(0) if call.past is not None else None
    if kw.get("return_scores"):
        res["scores"] = out.pop(0)
    if kw.get("return_finish"):
        res["finish"] = out.pop(0)
    assert not out, call.name
    return res, new_past


def differences(a, b):
    """What differs between two results of one call ([] when they are equal: ids, beam scores and Finish, all exactly)."""
    bad = []
    if a.keys() != b.keys():
        return [f"fields {sorted(a)} != {sorted(b)}"]
    if not torch.equal(a["ids"], b["ids"]):
        bad.append(f"ids {a['ids'].tolist()} != {b['ids'].tolist()}")
    if "scores" in a and not torch.equal(a["scores"], b["scores"]):
        bad.append(f"scores {a['scores'].tolist()} != {b['scores'].tolist()}")
    if "finish" in a:
        fa, fb = a["finish"], b["finish"]
        if not torch.equal(fa.kept, fb.kept) or fa.reason != fb.reason or fa.index != fb.index:
            bad.append(f"finish {fa} != {fb}")
    return bad


def generated(call, res):
    """Row b's generated ids of a (non-beam) result."""
    ids = res["ids"].tolist()
    return [row[n:] if call.ragged else row[max(call.lens):] for row, n in zip(ids, call.lens)]


def _distinct(cands, n, avoid=()):
    out = []
    for t in cands:
        if t not in out and t not in avoid:
            out.append(t)
        if len(out) == n:
            return out
    raise AssertionError(f"fewer than {n} distinct ids outside {list(avoid)} among {cands}")


def build_script(probe):
    """(units, pairs).  ``probe(call)`` gives the plain greedy ids (eos never, no rules) of the call's prompt, ``call.steps`` per
    row.  ``pairs``: name -> the names of calls that must be adjacent, in this order, on one pool key (check_pairs)."""
    units, pairs = [], {}

    def add(*calls):
        units.append(list(calls))

    # ---- key (2, 64, uniform): greedy with two eos ids that one row emits and the other does not, then the sampled calls
    g2 = Call("g2_probe", [9, 9], 12, prompt=1)
    r = probe(g2)
    e1 = _distinct(r[0][2:], 1, avoid=r[1])[0]                  # row 0 emits it early, row 1 never: the batch does not end
    e2 = _distinct(r[1][3:], 1, avoid=[e1])[0]
    add(Call("g2_eos1", [9, 9], 12, prompt=1, eos_token=e1))
    add(Call("g2_eos2", [9, 9], 12, prompt=1, eos_token=e2))
    samp = dict(temperature=0.8, top_k=20, top_p=0.9, eos_token=e2)
    add(Call("s2_seed5", [11, 11], 10, prompt=2, seed=5, **samp))
    add(Call("s2_seed6", [11, 11], 10, prompt=2, seed=6, **samp))
    add(Call("s2_seed5_again", [11, 11], 10, prompt=2, seed=5, **samp))
    pairs["sampled, another seed, the first seed again"] = ["s2_seed5", "s2_seed6", "s2_seed5_again"]
    add(Call("s2_other_values", [11, 11], 10, prompt=2, seed=5, temperature=1.2, top_k=0, top_p=0.5, eos_token=e2))
    add(Call("s2_transformers_min_p", [11, 11], 10, prompt=2, seed=5, temperature=0.9, top_k=50, top_p=0.8, min_p=0.05,
             sampler="transformers", eos_token=e2))
    pairs["sampled values, other values, transformers' sampler with min_p"] = ["s2_seed5_again", "s2_other_values",
                                                                              "s2_transformers_min_p"]

    # ---- key (4, 64, uniform): suppress ids swapped under one count, the rules after a long history, beam search, continuation
    p4 = Call("p4_plain", [7] * 4, 10, prompt=3)
    r = probe(p4)
    ab = _distinct([r[0][0], r[1][0]] + r[0] + r[1], 2)
    cd = _distinct([r[2][0], r[3][0]] + r[2] + r[3], 2, avoid=ab)
    add(Call("p4_suppress_ab", [7] * 4, 10, prompt=3, suppress_tokens=ab, min_new_tokens=2))
    add(Call("p4_suppress_cd", [7] * 4, 10, prompt=3, suppress_tokens=cd, min_new_tokens=2))
    add(p4)
    pairs["suppress {a, b}, {c, d}, processors off"] = ["p4_suppress_ab", "p4_suppress_cd", "p4_plain"]
    add(Call("h4_long_history", [5] * 4, 24, prompt=4))
    add(Call("h4_penalty_ngram", [6] * 4, 8, prompt=5, repetition_penalty=1.3, no_repeat_ngram_size=2))
    pairs["a long history, then repetition penalty and no-repeat n-grams"] = ["h4_long_history", "h4_penalty_ngram"]
    bm = Call("b4_probe", [10], 8, prompt=6)
    eb = probe(bm)[0][3]
    add(Call("b4_k4_scores", [10], 8, prompt=6, num_beams=4, return_scores=True, eos_token=eb))
    add(Call("b4_k2", [8, 8], 8, prompt=7, num_beams=2, eos_token=eb, length_penalty=0.8))
    pairs["beam k = 4 of one sample, then k = 2 of two"] = ["b4_k4_scores", "b4_k2"]
    add(Call("b4_k4_rules", [10], 8, prompt=6, num_beams=4, eos_token=eb, no_repeat_ngram_size=2, early_stopping=True))
    c4 = Call("c4_probe", [10] * 4, 6, prompt=8)
    ec = probe(c4)[0][2]                                        # row 0 is cut back to before it, the others keep a pending token
    add(Call("c4_returns_cache", [10] * 4, 6, prompt=8, past="new", eos_token=ec),
        Call("c4_continued", [5, 3, 6, 4], 6, ragged=True, prompt=9, past="cont", eos_token=ec),
        Call("c4_continued_again", [4] * 4, 6, prompt=10, past="cont", eos_token=ec, temperature=0.7, top_k=10, top_p=0.9, seed=3))
    pairs["beam k = 4, then greedy of 4 rows that returns its cache and is continued twice"] = [
        "b4_k4_rules", "c4_returns_cache", "c4_continued", "c4_continued_again"]

    # ---- key (2, 64, ragged): per-row stopping, a stale finish record, the returned cache and its successor
    st = Call("t2_probe", [9, 14], 12, ragged=True, prompt=11)
    r = probe(st)
    add(Call("t2_stop_a", [9, 14], 12, ragged=True, prompt=11, eos_token=[r[0][3]], stop_sequences=[r[1][4:6]], return_finish=True))
    add(Call("t2_stop_b", [9, 14], 12, ragged=True, prompt=11, eos_token=[r[1][2]], stop_sequences=[r[0][5:7]], return_finish=True))
    add(Call("t2_plain_eos", [9, 14], 12, ragged=True, prompt=11, eos_token=r[0][3]))
    pairs["stop sequences, others of the same counts, one eos under the reference's rule"] = ["t2_stop_a", "t2_stop_b", "t2_plain_eos"]
    add(Call("k2_returns_cache", [20, 13], 6, ragged=True, prompt=12, past="new", eos_token=[r[0][3]], stop_per_row=True),
        Call("k2_continued", [3, 8], 7, ragged=True, prompt=13, past="cont", eos_token=[r[0][3]], repetition_penalty=1.2))
    add(Call("k2_same_shape", [20, 13], 6, ragged=True, prompt=14))
    pairs["a call that returns its cache, then a call of its shape"] = ["k2_returns_cache", "k2_continued", "k2_same_shape"]

    # ---- key (1, 64, uniform): the eos id is a launch argument of the captured step, and the all-eos latch.  One row, so the
    # call ends at the first step that selects the eos id: a step replayed with the previous call's id ends the call elsewhere
    l1 = Call("l1_probe", [12], 16, prompt=15)
    r = probe(l1)[0]
    el = r[2]
    ef = _distinct(r[4:8], 1, avoid=r[:4])[0]                   # first selected later than el is
    add(Call("l1_ends_later", [12], 16, prompt=15, eos_token=ef))
    add(Call("l1_ends_early", [12], 16, prompt=15, eos_token=el))
    pairs["greedy, then another eos id"] = ["l1_ends_later", "l1_ends_early"]
    add(Call("l1_runs_on", [12], 10, prompt=15, eos_token=el, stop_on_eos=False))
    pairs["an early all-eos step, then stop_on_eos=False"] = ["l1_ends_early", "l1_runs_on"]

    # ---- keys (8, 64, ragged) and (8, 64, uniform)
    lens8 = [5, 40, 17, 9, 33, 21, 12, 28]
    add(Call("r8_ragged", lens8, 8, ragged=True, prompt=16))
    add(Call("u8_uniform", [40] * 8, 24, prompt=17))
    add(Call("r8_ragged_again", lens8, 8, ragged=True, prompt=16))
    pairs["ragged, uniform of the same (B, Smax), ragged again"] = ["r8_ragged", "u8_uniform", "r8_ragged_again"]

    return units, pairs


# pairs whose calls lie on two pool keys by design (the ragged and the uniform cache of one (B, Smax)) -- compared without the flag
TWO_KEYS = ("ragged, uniform of the same (B, Smax), ragged again",)


def check_pairs(units, pairs):
    """Every pair of ``pairs`` is present in the script: its calls adjacent, in order, on one pool key (a continuation stays on
    the key of the call whose cache it continues)."""
    flat = [c for u in units for c in u]
    names = [c.name for c in flat]
    assert len(set(names)) == len(names), "call names repeat"
    keys, last = {}, None
    for c in flat:
        last = c.key if c.key is not None else last
        keys[c.name] = last
    for what, seq in pairs.items():
        assert seq[0] in names, f"{what}: {seq[0]} is not in the script"
        i = names.index(seq[0])
        assert names[i: i + len(seq)] == seq, f"{what}: {seq} are not adjacent in the script ({names[i: i + len(seq)]})"
        ks = {keys[n][:2] if what in TWO_KEYS else keys[n] for n in seq}
        assert len(ks) == 1, f"{what}: the calls lie on pool keys {ks}"
        if what in TWO_KEYS:
            assert len({keys[n] for n in seq}) == 2, what
