"""Logits processors: the host statement (magma_amd.sampling.process_logits) against the installed transformers' processor
classes, bit for bit, and against transformers' generate() -- greedy and beam search -- on the tiny random GPT-J of
tests/test_beam_search_cpu.py driven by inputs_embeds; the argument checks of generate().  No GPU: the device kernel is tested
against the same host statement in tests/test_logits_processors_gpu.py."""
import math
from types import SimpleNamespace

import pytest
import torch

from magma_amd.sampling import beam_search, check_processor_args, generate, process_logits
from test_beam_search_cpu import EOS, V, _tiny_gptj

N_STEPS = 12
R = 4


def _scores(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=g) * 3          # both signs
    x[0, 5], x[1, 6], x[2, 7], x[3, 0] = 0.0, -0.0, float("-inf"), float("inf")
    return x


def _history(n_cols, seed):
    """(R, 12) tokens from a small alphabet (so that tokens, and n-grams, repeat), of which the first n_cols count."""
    g = torch.Generator().manual_seed(100 + seed)
    h = torch.randint(3, 9, (R, 12), generator=g)
    h[0, :] = torch.tensor([5, 6, 5, 6, 5, 6, 7, 5, 6, 5, 6, 5])      # the 2- and 3-gram ending the row occurred before
    h[1, :] = 6                                                        # one token, twelve times
    h[2, ::3] = V - 1
    h[3, 1::4] = 0
    return h[:, :n_cols].contiguous()


def _hf_chain(rules):
    """The transformers processors of ``rules`` (our argument names), in _get_logits_processor's order."""
    from transformers import (LogitsProcessorList, MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                              RepetitionPenaltyLogitsProcessor, SuppressTokensLogitsProcessor)
    chain = LogitsProcessorList()
    if "repetition_penalty" in rules:
        chain.append(RepetitionPenaltyLogitsProcessor(penalty=rules["repetition_penalty"]))
    if "no_repeat_ngram_size" in rules:
        chain.append(NoRepeatNGramLogitsProcessor(rules["no_repeat_ngram_size"]))
    if "min_new_tokens" in rules:
        chain.append(MinNewTokensLengthLogitsProcessor(0, rules["min_new_tokens"], EOS))
    if "suppress_tokens" in rules:
        chain.append(SuppressTokensLogitsProcessor(rules["suppress_tokens"]))
    return chain


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


ALONE = [dict(repetition_penalty=1.7), dict(repetition_penalty=0.5), dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=2),
         dict(no_repeat_ngram_size=3), dict(min_new_tokens=5), dict(suppress_tokens=[0, 3, 30, V - 1])]
CHAINED = [dict(repetition_penalty=1.7, no_repeat_ngram_size=n, min_new_tokens=5, suppress_tokens=[0, 3, 30, V - 1]) for n in (1, 2, 3)]


@pytest.mark.parametrize("rules", ALONE + CHAINED, ids=lambda r: "+".join(f"{k[:3]}{v}" for k, v in r.items()).replace(" ", ""))
def test_host_statement_equals_processor_classes(rules):
    pytest.importorskip("transformers")
    n = rules.get("no_repeat_ngram_size", 2)
    touched = False
    for step in sorted({0, 1, n - 1, n, 12}):
        x, hist = _scores(step), _history(step, step)
        ref = _hf_chain(rules)(hist, x.clone())
        got = process_logits(x, hist, step, eos_token=EOS, **rules)
        assert _same_bits(got, ref), (rules, step, (got != ref).nonzero())
        # a history wider than the step: only the first `step` columns count
        wide = torch.cat([hist, torch.full((R, 3), 11)], dim=1)
        assert _same_bits(process_logits(x, wide, step, eos_token=EOS, **rules), ref)
        touched = touched or not _same_bits(ref, x)
    assert touched          # the rule did something at one of the lengths


def test_penalty_is_applied_once_per_distinct_token():
    x = torch.full((1, V), 2.0)
    x[0, 9] = -2.0
    hist = torch.tensor([[6] * 11 + [9]])
    got = process_logits(x, hist, 12, repetition_penalty=1.3)
    assert float(got[0, 6]) == float(torch.tensor(2.0) / 1.3) and float(got[0, 9]) == float(torch.tensor(-2.0) * 1.3)
    assert float(process_logits(torch.full((1, V), float("-inf")), hist, 12, repetition_penalty=1.3)[0, 6]) == -math.inf


# ------------------------------------------------------------------------------------------- transformers' generate()
class _HostMagma(torch.nn.Module):
    """What sampling.generate() needs of a model, around an LM without device token selection (the host branch)."""

    class _LM(torch.nn.Module):
        def __init__(self, lm):
            super().__init__()
            self.inner, self.config = lm, lm.config

        def forward(self, cache_hint=None, reuse_cache=None, **kw):      # the engine's hints mean nothing to this LM
            return self.inner(**kw)

    def __init__(self, lm):
        super().__init__()
        self.lm, self.eos_token, self.image_token, self.tokenizer = self._LM(lm), EOS, V - 2, None


@pytest.fixture(scope="module")
def tiny():
    # seed 4: the plain greedy run loops on one token ("2 2 2 2") and reaches eos at steps 5 to 6 -- every rule has something
    # to change (at seed 3, the beam tests' model, greedy never emits eos within 12 steps)
    model = _tiny_gptj(seed=4, eos_bias=1.5)
    emb = torch.randn(3, 5, 32, generator=torch.Generator().manual_seed(11))
    return model, emb


def _cut(rows):
    """Every row: eos from its first eos on (transformers pads a finished row with the pad id = eos)."""
    rows = rows.clone()
    for r in rows:
        hits = (r == EOS).nonzero()
        if hits.numel():
            r[int(hits[0]):] = EOS
    return rows


def _pad(rows, n):
    return torch.cat([rows, torch.full((rows.shape[0], n - rows.shape[1]), EOS)], dim=1)


def _hf_generate(model, emb, k, rules):
    out = model.generate(inputs_embeds=emb, attention_mask=torch.ones(emb.shape[:2], dtype=torch.long), num_beams=k,
                         do_sample=False, max_new_tokens=N_STEPS, eos_token_id=EOS, pad_token_id=EOS, num_return_sequences=k,
                         output_scores=True, return_dict_in_generate=True, **rules)
    return out.sequences, (out.sequences_scores if k > 1 else None)


def _our_greedy(model, emb, rules):
    out = generate(_HostMagma(model), emb, max_steps=N_STEPS, temperature=0.0, eos_token=EOS, decode=False, **rules)
    return _pad(_cut(out[:, emb.shape[1]:]), N_STEPS)


def _our_beam(model, emb, k, rules):
    cache = {}
    emb_k = emb.repeat_interleave(k, dim=0)

    def step(rows, tokens):
        if rows is None:
            o = model(inputs_embeds=emb_k, use_cache=True)
        else:
            cache["past"].reorder_cache(rows)
            o = model(input_ids=tokens[:, None], past_key_values=cache["past"], use_cache=True)
        cache["past"] = o.past_key_values
        return o.logits[:, -1, :].float()

    with torch.no_grad():
        return beam_search(step, emb.shape[0], k, N_STEPS, EOS, 1.0, False, k, processors=check_processor_args(**rules))


def _biting_rules(plain):
    """The six cases, with values that change this fixture's plain greedy output ``plain`` (B, N_STEPS): the suppress list is
    taken from the tokens the plain run emits, min_new_tokens lies above its earliest eos."""
    first_eos = min(int((r == EOS).nonzero()[0]) for r in plain if bool((r == EOS).any()))
    emitted = sorted({int(r[0]) for r in plain} - {EOS})
    assert emitted and first_eos + 2 <= N_STEPS
    cases = {"penalty": dict(repetition_penalty=1.7), "ngram2": dict(no_repeat_ngram_size=2), "ngram1": dict(no_repeat_ngram_size=1),
             "min_new": dict(min_new_tokens=first_eos + 2), "suppress": dict(suppress_tokens=emitted)}
    cases["all"] = dict(repetition_penalty=1.7, no_repeat_ngram_size=2, min_new_tokens=first_eos + 2, suppress_tokens=emitted)
    return cases


CASES = ["penalty", "ngram2", "ngram1", "min_new", "suppress", "all"]


@pytest.mark.parametrize("case", CASES)
def test_greedy_equals_transformers_generate(tiny, case):
    pytest.importorskip("transformers")
    model, emb = tiny
    plain = _our_greedy(model, emb, {})
    assert torch.equal(plain, _pad(_hf_generate(model, emb, 1, {})[0], N_STEPS))
    rules = _biting_rules(plain)[case]
    ours = _our_greedy(model, emb, rules)
    ref = _pad(_hf_generate(model, emb, 1, rules)[0], N_STEPS)
    assert torch.equal(ours, ref), (rules, ours, ref)
    assert not torch.equal(ours, plain), (rules, "the rule left the output as it was")


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("case", CASES)
def test_beam_equals_transformers_generate(tiny, case, k):
    pytest.importorskip("transformers")
    model, emb = tiny
    rules = dict(_biting_rules(_our_greedy(model, emb, {}))[case])
    plain_seq, _, plain_len = _our_beam(model, emb, k, {})
    if "min_new_tokens" in rules:       # above the earliest eos of the plain BEAM run (its shortest hypothesis ends in eos)
        assert int(plain_len.min()) < N_STEPS
        rules["min_new_tokens"] = min(int(plain_len.min()) + 1, N_STEPS)
    seq, scores, _ = _our_beam(model, emb, k, rules)
    ref_seq, ref_scores = _hf_generate(model, emb, k, rules)
    assert seq.shape == ref_seq.shape and torch.equal(seq, ref_seq), (rules, seq, ref_seq)
    assert torch.allclose(scores, ref_scores.float(), rtol=0, atol=1e-5), (scores, ref_scores)
    assert seq.shape != plain_seq.shape or not torch.equal(seq, plain_seq), (rules, "the rule left the output as it was")


# ------------------------------------------------------------------------------------------------------- argument checks
def test_argument_validation():
    assert check_processor_args() is None and check_processor_args(1.0, 0, 0, []) is None
    assert check_processor_args(2, 0, 0, None) == dict(repetition_penalty=2.0, no_repeat_ngram_size=0, min_new_tokens=0,
                                                       suppress_tokens=())
    ok = check_processor_args(1.0, 0, 3, [EOS], vocab=V)           # eos may be listed while min_new_tokens is on
    assert ok["suppress_tokens"] == (EOS,) and ok["min_new_tokens"] == 3
    assert check_processor_args(suppress_tokens=list(range(1024)))["suppress_tokens"][-1] == 1023
    with pytest.raises(ValueError):
        check_processor_args(suppress_tokens=list(range(1025)))

    class _NoModel:            # the checks run before generate() touches the model
        eos_token = EOS
        training = False
        lm = SimpleNamespace(config=SimpleNamespace(vocab_size=V))

    emb = torch.zeros(1, 2, 8)
    bad = [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.5), dict(repetition_penalty="1.2"), dict(repetition_penalty=None),
           dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=17),
           dict(no_repeat_ngram_size=2.0), dict(min_new_tokens=-1), dict(min_new_tokens=1.5), dict(suppress_tokens=[-1]),
           dict(suppress_tokens=[V]), dict(suppress_tokens=[1.0]), dict(suppress_tokens=list(range(1025)))]
    for kw in bad:
        for beams in (1, 2):
            with pytest.raises(ValueError):
                generate(_NoModel(), emb, max_steps=2, num_beams=beams, **kw)
    with pytest.raises(TypeError):          # keyword-only, after the existing arguments
        generate(_NoModel(), emb, 2, 0.0, 0, 0.9, EOS, False, True, None, None, None, 1, 1.0, False, 1, False, None, False, 1.3)
