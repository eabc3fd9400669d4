"""Request streams on the host: the statement of a slot session's row test (magma_amd.sampling.slot_update) against stop_update
and at its boundaries, generate_stream's argument checks and refusals, and its host loop -- one solo generate() per request --
over the tiny random GPT-J of tests/test_stop_rows_cpu.py.  No GPU: the device kernels are tested against the same statement in
tests/test_stream_kernels_gpu.py, the engine's slot session in tests/test_stream_gpu.py."""
from types import SimpleNamespace

import pytest
import torch

from magma_amd.sampling import (REASON_EOS, REASON_LENGTH, REASON_NONE, REASON_STOP, StreamResult, generate, generate_stream,
                                slot_update, stop_update)
from test_beam_search_cpu import EOS, V, _tiny_gptj
from test_logits_processors_cpu import _HostMagma

NONE = [REASON_NONE, -1]


def test_slot_update_reduces_to_stop_update():
    """begin = 0, limit and Hc larger than the run: every step of a random run gives stop_update's rows and reasons."""
    g = torch.Generator().manual_seed(5)
    R, steps, Hc = 6, 20, 64
    hist = torch.randint(0, 6, (R, steps), generator=g)
    hist[0] = 7                 # a row that never finishes
    eos_ids, seqs = [5, 0], [[1, 2], [3], [2, 2, 4], [4, 1, 1, 3]]
    ring = torch.zeros(R, Hc, dtype=torch.int64)
    ring[:, :steps] = hist
    done_a = done_b = torch.zeros(R, dtype=torch.bool)
    begin, limit = torch.zeros(R, dtype=torch.int64), torch.full((R,), 1000)
    hits = set()
    for step in range(steps):
        done_a, why_a = stop_update(hist, step, done_a, eos_ids, seqs)
        done_b, why_b = slot_update(ring, step, done_b, begin, limit, eos_ids, seqs)
        assert torch.equal(done_a, done_b) and torch.equal(why_a, why_b), step
        hits |= {int(c) for c in why_a[:, 0]}
    assert {REASON_EOS, REASON_STOP} <= hits and not bool(done_a.all())


def test_slot_update_window_ring_and_budget():
    Hc = 8
    off = torch.zeros(1, dtype=torch.bool)
    # the previous occupant left 7 in column 2; the occupant's first token 9 sits in column 3: [7, 9] straddles begin
    ring = torch.tensor([[0, 0, 7, 9, 0, 0, 0, 0]])
    done, why = slot_update(ring, 3, off, [3], [10], [1], [[7, 9]])
    assert not bool(done[0]) and why.tolist() == [NONE]
    done, why = slot_update(ring, 3, off, [2], [10], [1], [[7, 9]])         # the same tokens, both the occupant's own
    assert bool(done[0]) and why.tolist() == [[REASON_STOP, 0]]
    # a sequence over the ring's wrap: the occupant began in column 6, step 17 is column 1 -> its tokens are columns 6, 7, 0, 1
    ring = torch.tensor([[5, 6, 0, 0, 0, 0, 3, 4]])
    done, why = slot_update(ring, 17, off, [6], [10], [1], [[9], [4, 5, 6], [3, 4, 5, 6]])
    assert bool(done[0]) and why.tolist() == [[REASON_STOP, 1]]             # the lowest matching index
    assert slot_update(ring, 17, off, [7], [10], [1], [[3, 4, 5, 6]])[1].tolist() == [NONE]     # one longer than the window
    # the budget: n = 4 tokens at step 17
    assert slot_update(ring, 17, off, [6], [4], [1], [])[1].tolist() == [[REASON_LENGTH, 0]]
    assert slot_update(ring, 17, off, [6], [5], [1], [])[1].tolist() == [NONE]
    assert slot_update(ring, 17, off, [6], [4], [6], [])[1].tolist() == [[REASON_EOS, 0]]       # eos and stop come first
    assert slot_update(ring, 17, off, [6], [4], [1], [[5, 6]])[1].tolist() == [[REASON_STOP, 0]]
    # limit = 1: the first token finishes the row whatever it is; a done row is not looked at
    assert slot_update(ring, 6, off, [6], [1], [1], [])[1].tolist() == [[REASON_LENGTH, 0]]
    assert slot_update(ring, 6, off, [6], [1], [3], [])[1].tolist() == [[REASON_EOS, 0]]
    done, why = slot_update(ring, 6, torch.ones(1, dtype=torch.bool), [6], [1], [3], [])
    assert bool(done[0]) and why.tolist() == [NONE]


class _NoModel:            # the checks run before generate_stream() touches the model
    eos_token = EOS
    training = False
    lm = SimpleNamespace(config=SimpleNamespace(vocab_size=V, max_position_embeddings=256))


def test_argument_checks_and_refusals():
    reqs = [torch.zeros(2, 8)]
    for kw in [dict(slots=17), dict(slots=0), dict(slots=2.0), dict(admit_rows=0), dict(slots=4, admit_rows=5), dict(every=0),
               dict(max_new_tokens=0), dict(max_prompt=0), dict(max_prompt=250, max_new_tokens=7), dict(max_new_tokens=256),
               dict(eos_token=[EOS, V]), dict(stop_sequences=[[1] * 17]), dict(eos_token=list(range(9))), dict(min_p=0.5),
               dict(sampler="other"), dict(temperature=0.7, min_p=0.1)]:
        with pytest.raises(ValueError):
            generate_stream(_NoModel(), reqs, **kw)
    refused = [dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(min_new_tokens=1), dict(suppress_tokens=[3]),
               dict(return_logprobs=True), dict(top_logprobs=2), dict(constraint=[[1, 2]]), dict(guidance_scale=1.5),
               dict(negative_embeddings=torch.zeros(1, 2, 8)), dict(num_beams=2), dict(return_scores=True), dict(num_beam_groups=2),
               dict(penalty_alpha=0.6), dict(past_key_values=object()), dict(return_past_key_values=True)]
    for kw in refused:
        with pytest.raises(NotImplementedError, match="not combined with generate_stream yet"):
            generate_stream(_NoModel(), reqs, **kw)
    generate_stream(_NoModel(), reqs, num_beams=1, repetition_penalty=1.0, constraint=None)      # generate()'s defaults pass
    with pytest.raises(TypeError):
        generate_stream(_NoModel(), reqs, max_steps=3)
    with pytest.raises(TypeError):          # keyword-only
        generate_stream(_NoModel(), reqs, 8)
    # the requests are checked as they are pulled, the error names the request
    model = _HostMagma(_tiny_gptj(seed=4, eos_bias=1.5))
    ok = torch.randn(3, 32, generator=torch.Generator().manual_seed(1))
    for bad in [torch.randn(9, 32), (ok, 5), (ok, 0), torch.zeros(2, 3, 32), "text"]:
        it = generate_stream(model, [ok, bad], max_new_tokens=4, max_prompt=8, decode=False)
        assert next(it).index == 0
        with pytest.raises(ValueError, match="request 1"):
            next(it)


def test_draw_counters_of_a_session_are_unique():
    """Sampled sessions: the admissions draw under counters of their own, so no (counter, row) pair is used twice -- not when the
    j-th staging row goes to slot j, and not when one round makes several staging passes."""
    from magma_amd.engine import SlotSession
    slots = 4
    schedule = [("admit", 4)] + [("step", slots)] * 3                     # first round at admit_rows = slots: staging row j -> slot j
    schedule += [("admit", 1), ("admit", 1), ("admit", 1)] + [("step", slots)] * 2      # three passes of one row in one round
    schedule += [("admit", 2)] + [("step", slots)] * 40 + [("admit", 4)] + [("step", slots)]
    draws = SlotSession.draw_counters(schedule)
    assert len(draws) == 4 + 3 + 2 + 4 + slots * 46 and len(set(draws)) == len(draws)
    assert all(0 <= c < 2 ** 32 for c, _ in draws)
    steps = {c for c, _ in draws if c < 2 ** 31}
    assert steps == set(range(1, 47))                                     # the token steps count from the session's state {1, -1}
    assert {c for c, _ in draws if c >= 2 ** 31} == {2 ** 32 - 1 - p for p in range(6)}     # one word per admission pass
    assert [SlotSession.admit_counter(p) for p in range(3)] == [-1, -2, -3]


class _Words:
    """A tokenizer stand-in: ids as words."""
    @staticmethod
    def decode(ids):
        return " ".join(str(int(t)) for t in ids)


def test_text_is_the_per_row_tail_of_generate():
    """decode=True: StreamResult.text is what generate(decode=True) gives for the request alone -- the eos dropped, a stop
    sequence kept, image tokens removed."""
    model = _HostMagma(_tiny_gptj(seed=4, eos_bias=1.5))
    model.tokenizer = _Words()
    g = torch.Generator().manual_seed(11)
    prompts = [torch.randn(n, 32, generator=g) for n in (5, 1, 7, 3, 5, 2)]
    kw = dict(eos_token=[EOS, V - 3])
    limits = [3, 8, 8, 8, 2, 8]
    got = list(generate_stream(model, list(zip(prompts, limits)), max_new_tokens=8, max_prompt=8, **kw))
    reasons = set()
    for r, p, n in zip(got, prompts, limits):
        want, fin = generate(model, p[None], max_steps=n, stop_per_row=True, return_finish=True, temperature=0.0, decode=True, **kw)
        ids = r.tokens.tolist()
        assert r.text == want[0] and r.reason == fin.reason[0]
        assert r.text == _Words.decode([t for t in (ids[:-1] if r.reason == "eos" else ids) if t != model.image_token])
        reasons.add(r.reason)
    assert reasons == {"eos", "length"}, [(r.reason, r.tokens.tolist()) for r in got]


def test_host_loop_yields_every_request_once_with_the_solo_ids():
    """An LM object without device token selection: one solo generate() per request, lazily, in order."""
    model = _HostMagma(_tiny_gptj(seed=4, eos_bias=1.5))
    g = torch.Generator().manual_seed(11)
    lens, limits = [5, 1, 7, 3, 5, 2], [12, 1, 3, 12, 6, None]
    prompts = [torch.randn(1, n, 32, generator=g) if i % 2 else torch.randn(n, 32, generator=g) for i, n in enumerate(lens)]
    plain = [generate(model, p.view(1, -1, 32), max_steps=12, temperature=0.0, eos_token=EOS, decode=False, stop_on_eos=False)[0, n:].tolist()
             for p, n in zip(prompts, lens)]
    seq = next(row[t:t + 2] for row in plain for t in range(2, 8) if EOS not in row[:t + 2])      # a request's own two tokens
    pulled = []

    def stream():
        for i, (p, n) in enumerate(zip(prompts, limits)):
            pulled.append(i)
            yield p if n is None else (p, n)

    it = generate_stream(model, stream(), max_new_tokens=12, max_prompt=8, eos_token=[EOS, V - 3], stop_sequences=[seq], decode=False)
    assert pulled == []                                      # nothing runs before the first next()
    got = []
    for res in it:
        assert isinstance(res, StreamResult) and pulled == list(range(res.index + 1))         # one item per finished request
        got.append(res)
    assert [r.index for r in got] == list(range(len(prompts)))
    reasons = set()
    for r, p, n, limit in zip(got, prompts, lens, limits):
        out, fin = generate(model, p.view(1, -1, 32), max_steps=limit or 12, eos_token=[EOS, V - 3], stop_sequences=[seq],
                            stop_per_row=True, return_finish=True, temperature=0.0, decode=False)
        assert r.tokens.dtype == torch.int64 and r.tokens.device.type == "cpu"
        assert r.tokens.tolist() == out[0, n: n + int(fin.kept[0])].tolist() and 1 <= len(r.tokens) <= (limit or 12)
        assert (r.reason, r.reason_index, r.text, r.slot) == (fin.reason[0], fin.index[0], None, None)
        reasons.add(r.reason)
    assert reasons == {"eos", "stop", "length"}, [(r.reason, r.tokens.tolist()) for r in got]
