"""Beam search: the host statement (magma_amd.sampling.beam_search) against the installed transformers'
GenerationMixin._beam_search on a tiny random GPT-J driven by inputs_embeds, and the argument checks of generate().
No GPU: the device kernels are tested against the same host statement in tests/test_beam_search_gpu.py."""
import pytest
import torch

from magma_amd.sampling import beam_search, check_beam_args, generate

V, EOS, N_STEPS = 48, 7, 9


def _tiny_gptj(seed, eos_bias):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.GPTJConfig(vocab_size=V, n_embd=32, n_layer=2, n_head=4, rotary_dim=4, n_positions=64,
                                  bos_token_id=EOS, eos_token_id=EOS, pad_token_id=EOS, attn_implementation="eager")
    torch.manual_seed(seed)
    model = transformers.GPTJForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.normal_(0.0, 0.3)
        model.lm_head.bias[EOS] += eos_bias        # eos is reached within a few steps, at different steps per beam
    return model


def _hf_beam(model, emb, k, lp, es, n_ret, monkeypatch):
    from transformers import GenerationConfig
    from transformers.generation.configuration_utils import GenerationMode
    if k == 1:        # transformers runs greedy search at num_beams = 1: ask for its beam search explicitly
        monkeypatch.setattr(GenerationConfig, "get_generation_mode", lambda self, *a, **kw: GenerationMode.BEAM_SEARCH)
    out = model.generate(inputs_embeds=emb, attention_mask=torch.ones(emb.shape[:2], dtype=torch.long), num_beams=k,
                         do_sample=False, max_new_tokens=N_STEPS, eos_token_id=EOS, pad_token_id=EOS, length_penalty=lp,
                         early_stopping=es, num_return_sequences=n_ret, output_scores=True, return_dict_in_generate=True)
    monkeypatch.undo()
    return out.sequences, out.sequences_scores if k > 1 or out.get("sequences_scores") is not None else None


def _ours(model, emb, k, lp, es, n_ret):
    B = emb.shape[0]
    cache = {}
    emb_k = emb.repeat_interleave(k, dim=0)

    def step(rows, tokens):
        if rows is None:
            o = model(inputs_embeds=emb_k, use_cache=True)
        else:
            past = cache["past"]
            past.reorder_cache(rows)
            o = model(input_ids=tokens[:, None], past_key_values=past, use_cache=True)
        cache["past"] = o.past_key_values
        return o.logits[:, -1, :].float()

    with torch.no_grad():
        return beam_search(step, B, k, N_STEPS, EOS, lp, es, n_ret)


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("lp", [1.0, 0.0, 2.0, -0.5])
@pytest.mark.parametrize("es", [True, False, "never"])
@pytest.mark.parametrize("ret", ["one", "all"])
def test_host_statement_equals_transformers(k, lp, es, ret, monkeypatch):
    n_ret = 1 if ret == "one" else k
    model = _tiny_gptj(seed=3, eos_bias=1.5)
    g = torch.Generator().manual_seed(11)
    emb = torch.randn(3, 5, 32, generator=g)
    ref_seq, ref_scores = _hf_beam(model, emb, k, lp, es, n_ret, monkeypatch)
    seq, scores, lens = _ours(model, emb, k, lp, es, n_ret)
    assert seq.shape == ref_seq.shape and torch.equal(seq, ref_seq), (seq, ref_seq)
    if ref_scores is not None:
        assert torch.allclose(scores, ref_scores.float(), rtol=0, atol=1e-5), (scores, ref_scores)
    # every returned hypothesis ends in eos or runs to max_steps; its tokens after its length are eos
    for row, n in zip(seq, lens.tolist()):
        assert 1 <= n <= N_STEPS and (row[n - 1] == EOS or n == N_STEPS) and bool((row[n:] == EOS).all())


def test_eos_actually_reached():
    """The fixture must exercise the finish rule: some hypotheses end in eos before max_steps, at different lengths."""
    model = _tiny_gptj(seed=3, eos_bias=1.5)
    emb = torch.randn(3, 5, 32, generator=torch.Generator().manual_seed(11))
    _, _, lens = _ours(model, emb, 4, 1.0, "never", 4)
    assert (lens < N_STEPS).any() and len(set(lens.tolist())) > 1, lens


def test_argument_validation():
    assert check_beam_args(4, 2, "never") == "never" and check_beam_args(1, 1, 0) is False
    for nb, nr, es in [(0, 1, False), (-2, 1, False), (17, 1, False), (2, 3, False), (4, 0, False), (2, 1, "sometimes"),
                       (2, 1, 0.5), (2.0, 1, False)]:
        with pytest.raises(ValueError):
            check_beam_args(nb, nr, es)

    class _NoModel:            # the checks run before generate() touches the model
        eos_token = EOS
        training = False

    emb = torch.zeros(1, 2, 8)
    for kw in [dict(num_beams=2, num_return_sequences=3), dict(num_beams=0), dict(num_beams=17),
               dict(num_beams=2, early_stopping="soon")]:
        with pytest.raises(ValueError):
            generate(_NoModel(), emb, max_steps=2, **kw)


def test_cache_keeps_its_length_and_beam_state_is_plain():
    """len(past_key_values) is the number of layers, as before beam search; the beam state is an ordinary object."""
    from magma_amd.engine import BeamBuffers, KVCache
    cache = KVCache(3, 4, 1, 16, "cpu")
    assert len(cache) == 3 and cache.beam is None
    cache.beam = BeamBuffers(cache, 2, torch.zeros(4, dtype=torch.int64))
    assert cache.beam and cache.beam.k == 2 and cache.beam.B == 2 and len(cache) == 3
