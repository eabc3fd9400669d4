"""The frame generate() shares between its selection modes (magma_amd.sampling): the one layout of the returned ids against the
three statements it replaced, the eval-mode block that gives the model back in the mode it came in -- after an exception too --,
the defaults of the poll interval and of the sampling seed, and the calls the one device loop makes for greedy, beam and
contrastive search, recorded from a stand-in for the engine's LM.  No GPU: the engine itself runs the loop in the *_gpu.py tests."""
from types import SimpleNamespace

import pytest
import torch

from magma_amd.sampling import eval_mode, generate, generate_stream, layout_ids, poll_every
from test_beam_search_cpu import EOS, V, _tiny_gptj
from test_logits_processors_cpu import _HostMagma

IMAGE = V - 2


# ------------------------------------------------------------------------------------------------------------------- the layout
def _old_device_loop(tokens, s, lengths, image_token, eos_token):
    b, n_gen = tokens.shape
    dev = tokens.device
    out = torch.full((b, s + n_gen), eos_token, dtype=torch.long, device=dev)
    if lengths is not None:
        lens = lengths.to(dev, non_blocking=True)[:, None]
        out.masked_fill_(torch.arange(s + n_gen, device=dev)[None, :] < lens, image_token)
        out.scatter_(1, lens + torch.arange(n_gen, device=dev)[None, :], tokens)
    else:
        out[:, :s] = image_token
        out[:, s:] = tokens
    return out


def _old_beam(toks, s, lengths, image_token, eos_token, b, n_ret):
    dev = toks.device
    n = toks.shape[1]
    out = torch.full((b * n_ret, s + n), eos_token, dtype=torch.long, device=dev)
    if lengths is None:
        out[:, :s] = image_token
        out[:, s:] = toks
    else:
        lens_r = lengths.to(dev).repeat_interleave(n_ret)[:, None]
        out.masked_fill_(torch.arange(s + n, device=dev)[None, :] < lens_r, image_token)
        out.scatter_(1, lens_r + torch.arange(n, device=dev)[None, :], toks)
    return out


def _old_contrastive(toks, s, lengths, image_token, eos_token, b):
    dev = toks.device
    n = toks.shape[1]
    out = torch.full((b, s + n), eos_token, dtype=torch.long, device=dev)
    if lengths is None:
        out[:, :s] = image_token
        out[:, s:] = toks
    else:
        lens = lengths.to(dev)[:, None]
        out.masked_fill_(torch.arange(s + n, device=dev)[None, :] < lens, image_token)
        out.scatter_(1, lens + torch.arange(n, device=dev)[None, :], toks)
    return out


@pytest.mark.parametrize("n", [0, 4])
@pytest.mark.parametrize("repeat", [1, 3])
@pytest.mark.parametrize("ragged", [False, True])
def test_layout_ids_is_the_three_statements_it_replaced(ragged, repeat, n):
    b, s = 4, 6
    lengths = torch.tensor([s, 1, 3, 5]) if ragged else None           # a full row, a row of one position
    tokens = torch.randint(0, V - 2, (b * repeat, n), generator=torch.Generator().manual_seed(n + repeat))
    got = layout_ids(tokens, s, lengths, IMAGE, EOS, repeat)
    assert got.dtype == torch.int64 and got.shape == (b * repeat, s + n)
    assert torch.equal(got, _old_beam(tokens, s, lengths, IMAGE, EOS, b, repeat))
    if repeat == 1:
        assert torch.equal(got, _old_device_loop(tokens, s, lengths, IMAGE, EOS))
        assert torch.equal(got, _old_contrastive(tokens, s, lengths, IMAGE, EOS, b))
    # and by its meaning: the image token for the row's prompt, its tokens, eos behind them
    for r in range(b * repeat):
        at = int(lengths[r // repeat]) if ragged else s
        assert got[r, :at].tolist() == [IMAGE] * at and torch.equal(got[r, at:at + n], tokens[r])
        assert got[r, at + n:].tolist() == [EOS] * (s - at)


# ---------------------------------------------------------------------------------------------------------------- the eval mode
class _RaisesOnThirdCall(torch.nn.Module):
    def __init__(self, lm):
        super().__init__()
        self.lm, self.config, self.calls = lm, lm.config, 0

    def forward(self, **kw):
        self.calls += 1
        if self.calls == 3:
            raise RuntimeError("the third call is refused")
        return self.lm(**kw)


ENTRIES = {"greedy": dict(temperature=0.0), "beam": dict(num_beams=2), "contrastive": dict(penalty_alpha=0.6, top_k=2)}


@pytest.fixture(scope="module")
def tiny():
    return _tiny_gptj(seed=4, eos_bias=1.5), torch.randn(2, 5, 32, generator=torch.Generator().manual_seed(11))


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_an_exception_leaves_the_model_in_the_mode_it_came_in(tiny, entry):
    lm, emb = tiny
    kw = dict(max_steps=6, decode=False, stop_on_eos=False, **ENTRIES[entry])
    model = _HostMagma(_RaisesOnThirdCall(lm)).train()
    with pytest.raises(RuntimeError, match="third call"):
        generate(model, emb, **kw)
    assert model.training is True and model.lm.inner.calls == 3
    model = _HostMagma(_RaisesOnThirdCall(lm)).eval()
    with pytest.raises(RuntimeError, match="third call"):
        generate(model, emb, **kw)
    assert model.training is False


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_normal_call_restores_the_mode(tiny, entry):
    lm, emb = tiny
    seen = []
    hook = lm.register_forward_pre_hook(lambda mod, args: seen.append(mod.training))
    try:
        for training in (True, False):
            model = _HostMagma(lm).train(training)
            out = generate(model, emb, max_steps=3, decode=False, stop_on_eos=False, **ENTRIES[entry])
            assert model.training is training and lm.training is training and out.shape[0] == 2 and out.shape[1] <= 5 + 3
    finally:
        hook.remove()
    assert seen and not any(seen)               # every call of the LM ran in eval mode


def test_eval_mode_restores_after_an_exception():
    m = torch.nn.Linear(2, 2)
    with pytest.raises(KeyError):
        with eval_mode(m):
            assert not m.training
            raise KeyError("x")
    assert m.training
    with eval_mode(m.eval()):
        pass
    assert not m.training


# ------------------------------------------------------------------------------------------- the device loop, the poll, the seed
class _Record:
    """The device's {step, first all-eos step} record: notes the step of the loop at which the host reads its second entry."""

    def __init__(self, lm):
        self.lm = lm

    def __getitem__(self, i):
        assert i == 1
        self.lm.looks.append(len(self.lm.calls))
        return self.lm.all_eos


class _EngineLM:
    """What generate()'s device loop needs of the engine's LM: it records every call's keywords and every look at the record."""
    device_token_selection = True

    def __init__(self, all_eos=-1):
        self.calls, self.looks, self.all_eos = [], [], all_eos
        self.config = SimpleNamespace(vocab_size=V, head_rows=None)
        self.engine = SimpleNamespace(V=V, beam_results=self.beam_results)

    def __call__(self, **kw):
        self.calls.append(kw)
        if kw.get("inputs_embeds") is not None:
            rows = kw["inputs_embeds"].shape[0]
            self.past = SimpleNamespace(history=torch.arange(rows)[:, None] * 100 + torch.arange(32)[None, :])
            return SimpleNamespace(past_key_values=self.past, eos_state=_Record(self))
        assert kw["past_key_values"] is self.past
        return SimpleNamespace(past_key_values=self.past, eos_state=_Record(self))

    def beam_results(self, past, n_ret):
        assert past is self.past
        rows = past.history.shape[0] // self.k * n_ret
        return torch.full((rows, 3), 9), torch.arange(rows, dtype=torch.float32), torch.full((rows,), 3)


def _engine_model(**kw):
    lm = _EngineLM(**kw)
    return SimpleNamespace(lm=lm, eos_token=EOS, image_token=IMAGE, training=False, eval=lambda: None, train=lambda mode: None)


STEP = dict(input_ids=None, use_cache=True, feed_back=True)


def _prefill_and_steps(model, rows, n_steps, lengths):
    """The keywords of the loop's calls, whatever the selection mode: one prefill over ``rows`` rows into a pooled cache, then
    ``n_steps`` fed-back steps under the same plan and nothing else."""
    first, rest = model.lm.calls[0], model.lm.calls[1:]
    # (``seed`` is None -- the keyword's default -- where no sampling stream is drawn from)
    plan = first["plan"]
    assert set(first) == {"inputs_embeds", "use_cache", "past_key_values", "cache_hint", "reuse_cache", "eos_token", "seed", "plan",
                          "lengths"}
    assert first["inputs_embeds"].shape[0] == rows and first["use_cache"] is True and first["past_key_values"] is None
    assert first["reuse_cache"] is True and first["eos_token"] == EOS
    assert (first["lengths"] is None) if lengths is None else first["lengths"].tolist() == lengths
    assert len(rest) == n_steps
    for kw in rest:
        assert set(kw) == set(STEP) | {"past_key_values", "plan"} and all(kw[k] is v for k, v in STEP.items())
        assert kw["plan"] is plan and kw["past_key_values"] is model.lm.past
    return first, plan


def test_device_loop_greedy_calls_and_poll(monkeypatch):
    emb = torch.zeros(2, 4, 8)
    monkeypatch.setenv("MAGMA_EOS_CHECK_EVERY", "3")
    model = _engine_model()
    out = generate(model, emb, max_steps=7, temperature=0.0, decode=False, lengths=[4, 2])
    first, plan = _prefill_and_steps(model, 2, 6, [4, 2])            # the prefill is step 0 of 7
    assert first["cache_hint"] == 7 and first["seed"] is None and plan.mode is None and not plan.is_beam
    assert model.lm.looks == [3, 6, 7]                               # MAGMA_EOS_CHECK_EVERY = 3, and the last step
    assert out.shape == (2, 4 + 7) and out[0, 4:].tolist() == list(range(7)) and out[1, 2:9].tolist() == list(range(100, 107))
    model = _engine_model()
    generate(model, emb, max_steps=7, temperature=0.0, decode=False, eos_check_every=2)
    assert model.lm.looks == [2, 4, 6, 7]                            # the explicit argument wins
    assert poll_every() == 3 and poll_every(5) == 5
    monkeypatch.delenv("MAGMA_EOS_CHECK_EVERY")
    assert poll_every() == 8
    model = _engine_model()
    generate(model, emb, max_steps=4, temperature=0.0, decode=False, stop_on_eos=False)
    assert model.lm.looks == [] and len(model.lm.calls) == 4         # nobody looks when nothing would stop the loop
    model = _engine_model(all_eos=1)                                 # every row emitted eos at step 1: seen at the look of step 4
    out = generate(model, emb, max_steps=9, temperature=0.0, decode=False, eos_check_every=4)
    assert model.lm.looks == [4] and len(model.lm.calls) == 4 and out.shape == (2, 4 + 2)


def test_device_loop_beam_calls_and_poll():
    emb = torch.arange(2.0)[:, None, None].expand(2, 4, 8)
    model = _engine_model()
    model.lm.k = 3
    out, scores = generate(model, emb, max_steps=5, num_beams=3, num_return_sequences=2, return_scores=True, decode=False,
                           eos_check_every=2, lengths=[4, 1], stop_on_eos=False)
    first, plan = _prefill_and_steps(model, 6, 4, [4, 4, 4, 1, 1, 1])
    assert first["inputs_embeds"][:, 0, 0].tolist() == [0, 0, 0, 1, 1, 1] and first["cache_hint"] == 5 and first["seed"] is None
    assert plan.is_beam and plan.mode == ("beam", 3, 1.0, False, 5)
    assert model.lm.looks == [2, 4, 5]                               # beam search always looks
    assert out.shape == (4, 4 + 3) and scores.tolist() == [0, 1, 2, 3]
    assert out.tolist() == [[IMAGE] * 4 + [9] * 3] * 2 + [[IMAGE] + [9] * 3 + [EOS] * 3] * 2
    model = _engine_model(all_eos=0)
    model.lm.k = 2
    out = generate(model, emb, max_steps=8, num_beams=2, decode=False, eos_check_every=3)
    assert model.lm.looks == [3] and len(model.lm.calls) == 3 and out.shape == (2, 4 + 3)    # the record ends the loop, cuts nothing


def test_device_loop_contrastive_calls_and_poll():
    emb = torch.arange(2.0)[:, None, None].expand(2, 4, 8)
    model = _engine_model()
    out = generate(model, emb, max_steps=5, penalty_alpha=0.6, top_k=2, decode=False, eos_check_every=2, lengths=[3, 4])
    first, plan = _prefill_and_steps(model, 4, 5, [3, 3, 4, 4])       # the prefill selects nothing: 5 token steps follow it
    assert first["inputs_embeds"][:, 0, 0].tolist() == [0, 0, 1, 1] and first["cache_hint"] == 5 and first["seed"] is None
    assert plan.is_contrast and plan.mode == ("contrast", 2, 0.6)
    assert model.lm.looks == [3, 5, 6]                                # after token steps 2, 4 and 5 (the prefill is call 1)
    assert out.shape == (2, 4 + 5)                                    # the history of every sample's first row
    assert out[0].tolist() == [IMAGE] * 3 + [0, 1, 2, 3, 4] + [EOS] and out[1].tolist() == [IMAGE] * 4 + [200, 201, 202, 203, 204]
    model = _engine_model()
    generate(model, emb, max_steps=3, penalty_alpha=0.6, top_k=2, decode=False, stop_on_eos=False)
    assert model.lm.looks == [] and len(model.lm.calls) == 4
    model = _engine_model(all_eos=0)
    out = generate(model, emb, max_steps=6, penalty_alpha=0.6, top_k=2, decode=False, eos_check_every=2)
    assert model.lm.looks == [3] and out.shape == (2, 4 + 1)


PARENT_SEED = 900450186894289455


def test_the_seed_of_a_sampled_call_is_drawn_where_it_was():
    """The value: what the commit before this module drew for the same call after torch.manual_seed(0), recorded there once."""
    emb = torch.zeros(2, 4, 8)
    for kw in (dict(temperature=0.7), dict(temperature=0.7, sampler="transformers", top_p=0.8, min_p=0.1)):
        model = _engine_model()
        torch.manual_seed(0)
        generate(model, emb, max_steps=2, decode=False, **kw)
        assert model.lm.calls[0]["seed"] == PARENT_SEED
        after = torch.randint(0, 2 ** 62, (1,))
        torch.manual_seed(0)
        torch.randint(0, 2 ** 62, (1,))
        assert torch.equal(after, torch.randint(0, 2 ** 62, (1,)))      # exactly one draw was taken
    assert model.lm.calls[0]["plan"].mode == ("warp", 0.7, 0, 0.8, 0.1)
    model = _engine_model()
    generate(model, emb, max_steps=2, decode=False, temperature=0.7, seed=5)
    assert model.lm.calls[0]["seed"] == 5 and model.lm.calls[0]["plan"].mode == (0.7, 0, 0.9)
    model = _engine_model()
    model.lm.config.max_position_embeddings, model.lm.engine.device = 256, "cpu"
    torch.manual_seed(0)
    generate_stream(model, [], temperature=0.7, max_new_tokens=4, max_prompt=8)      # a stream draws its seed when the call is made
    after = torch.randint(0, 2 ** 62, (1,))
    torch.manual_seed(0)
    assert int(torch.randint(0, 2 ** 62, (1,))) == PARENT_SEED and torch.equal(after, torch.randint(0, 2 ** 62, (1,)))
