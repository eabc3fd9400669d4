"""Classifier-free guidance (DESIGN.md "Classifier-free guidance"): the host statement (magma_amd.sampling.guide_logits) against
the installed transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor, its plausibility cut, the argument checks of
generate(), and the host branch of generate(guidance_scale=...) on the tiny random GPT-J of tests/test_beam_search_cpu.py.
No GPU: the device kernels are tested against the same statement in tests/test_guidance_gpu.py.

The value bound.  The statement is float64; whoever computes out = u + s (c - u) in fp32 from fp32 log_softmax values c', u' with
|c' - c| <= E(c), |u' - u| <= E(u) (E: the bound of tests/test_logprobs_gpu.py, 2^-22 max(1, |lp|) + (ceil(V / 1024) + 16) 2^-24)
forms  u' + s (c' - u') = (1 - s) u' + s c',  which carries the two log_softmax errors scaled by their coefficients, s E(c) and
|1 - s| E(u); one rounding of the product s (c' - u') (the difference of two fp32 numbers is itself rounded once; both are
covered by 2^-23 max(1, |s (c - u)|) each, as s >= 0 scales the difference's rounding too) and one rounding of the final sum,
2^-23 max(1, |out|).  Together, per element:

    G = s E(c) + |1 - s| E(u) + 2^-22 max(1, |s (c - u)|, |out|)

Measured here: transformers' own fp32 arithmetic reaches at most 0.35 G on these inputs (the test prints the figure)."""
import math
from types import SimpleNamespace

import pytest
import torch

from magma_amd.sampling import check_guidance_args, generate, guide_logits
from test_beam_search_cpu import EOS, V as TINY_V, _tiny_gptj

NEG_INF = float("-inf")


def lp_bound(lp, V):
    """E of tests/test_logprobs_gpu.py."""
    return 2.0 ** -22 * lp.abs().clamp(min=1.0) + (math.ceil(V / 1024) + 16) * 2.0 ** -24


def guidance_bound(cond, uncond, scale):
    """G per element (float64), from the float64 log_softmax of the fp32 inputs."""
    V = cond.shape[-1]
    c, u = torch.log_softmax(cond.double(), -1), torch.log_softmax(uncond.double(), -1)
    out = u + scale * (c - u)
    fin = torch.where(torch.isfinite(out), out, torch.zeros_like(out))
    prod = torch.where(torch.isfinite(c), scale * (c - u), torch.zeros_like(c))
    Ec = lp_bound(torch.where(torch.isfinite(c), c, torch.zeros_like(c)), V)
    rnd = 2.0 ** -22 * torch.maximum(torch.maximum(prod.abs(), fin.abs()), torch.ones_like(fin))
    return scale * Ec + abs(1.0 - scale) * lp_bound(u, V) + rnd


def _pair(R, V, spread, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, V, generator=g) * spread, torch.randn(R, V, generator=g) * spread


# ------------------------------------------------------------------------------------------------ the rule and transformers
@pytest.mark.parametrize("V", [7, 64, 1025, 50258])
@pytest.mark.parametrize("spread", [1, 3, 10])
def test_statement_equals_transformers_processor(V, spread):
    pytest.importorskip("transformers")
    from transformers import UnbatchedClassifierFreeGuidanceLogitsProcessor
    worst = 0.0
    for scale in (0.0, 0.5, 1.5, 3.0, 7.5):
        cond, uncond = _pair(3, V, spread, seed=V + 7 * spread)
        hf = UnbatchedClassifierFreeGuidanceLogitsProcessor(scale, model=None)
        hf.get_unconditional_logits = lambda input_ids: uncond[:, None, :]
        ref = hf(torch.zeros(3, 1, dtype=torch.int64), cond.clone())
        assert ref.dtype == torch.float32
        got = guide_logits(cond, uncond, scale)
        assert got.dtype == torch.float64 and got.shape == cond.shape
        ratio = float(((ref.double() - got).abs() / guidance_bound(cond, uncond, scale)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (V, spread, scale, ratio)
    print(f"V={V} spread={spread}: transformers fp32 against the statement, max err / G = {worst:.3f}")
    assert worst > 0.0          # the two are different arithmetic: the bound is compared with something


def test_statement_edges():
    cond, uncond = _pair(2, 33, 3, seed=5)
    cond[0, 4] = NEG_INF
    for scale in (0.0, 1.0, 2.5):
        out = guide_logits(cond, uncond, scale)
        assert float(out[0, 4]) == NEG_INF and int(torch.isinf(out).sum()) == 1 and not bool(torch.isnan(out).any()), scale
    one, c = guide_logits(cond, uncond, 1.0), torch.log_softmax(cond.double(), -1)
    assert float((one - c)[torch.isfinite(c)].abs().max()) < 1e-13          # (u + (c - u) rounds twice in float64)
    assert torch.equal(guide_logits(cond, uncond, 0.0)[1], torch.log_softmax(uncond.double(), -1)[1])
    bad = uncond.clone()
    bad[1, 0] = NEG_INF
    with pytest.raises(ValueError):
        guide_logits(cond, bad, 2.0)
    for kw in (dict(guidance_scale=-1.0), dict(guidance_scale=float("nan")), dict(guidance_scale=float("inf")),
               dict(guidance_scale=2.0, guidance_min_p=1.5), dict(guidance_scale=2.0, guidance_min_p=-0.1)):
        with pytest.raises(ValueError):
            guide_logits(cond, uncond, **kw)
    with pytest.raises(ValueError):
        guide_logits(cond, uncond[:1], 2.0)


# --------------------------------------------------------------------------------------------------- the plausibility cut
@pytest.mark.parametrize("V", [7, 1025, 50258])
@pytest.mark.parametrize("min_p", [0.5, 0.1, 1e-3])
def test_cut_keeps_the_plausible_tokens(V, min_p):
    cond, uncond = _pair(3, V, 3, seed=V)
    d = cond.double() - cond.double().max(-1, keepdim=True).values
    near = (d - math.log(min_p)).abs() < 1e-3           # margins around the threshold >= 1e-3
    cond = torch.where(near, cond - 4e-3, cond)
    d = cond.double() - cond.double().max(-1, keepdim=True).values
    assert float((d - math.log(min_p)).abs().min()) >= 1e-3
    p = torch.softmax(cond.double(), -1)
    want = p >= min_p * p.max(-1, keepdim=True).values
    for scale in (0.0, 3.0):
        out = guide_logits(cond, uncond, scale, min_p)
        assert torch.equal(out > NEG_INF, want), (V, min_p, scale)
        free = guide_logits(cond, uncond, scale)
        assert torch.equal(out[want], free[want])           # a kept token keeps the rule's value
    assert bool(want.any(-1).all()) and (V == 7 or not bool(want.all()))


def test_cut_ties_maxima_and_the_bound_in_fp32():
    V = 40
    cond, uncond = _pair(2, V, 2, seed=9)
    cond = cond - cond.max(-1, keepdim=True).values - 1.0   # every entry <= -1 ...
    cond[:, 3] = 0.0
    cond[0, 17] = 0.0                                       # ... a row with two maxima, a row with one
    out = guide_logits(cond, uncond, 7.5, 1.0)              # guidance_min_p = 1 keeps exactly the maxima
    assert (out > NEG_INF).nonzero().tolist() == [[0, 3], [0, 17], [1, 3]]
    # ties AT the threshold stay: the fp32 difference is compared with the fp32 rounding of the float64 log
    min_p = 0.1
    bound = torch.tensor(min_p, dtype=torch.float64).log().to(torch.float32)
    cond[0, 5], cond[0, 6] = bound, torch.nextafter(bound, torch.tensor(NEG_INF))
    cond[1, 5], cond[1, 6] = torch.nextafter(bound, torch.tensor(0.0)), bound * 2
    kept = guide_logits(cond, uncond, 2.0, min_p) > NEG_INF
    assert kept[0, 5] and not kept[0, 6] and kept[1, 5] and not kept[1, 6]
    assert bool(kept[:, 3].all())                           # the row maximum always survives


# ------------------------------------------------------------------------------------------------------ argument checks
class _NoModel:            # the checks run before generate() touches the model
    eos_token = EOS
    training = False
    tokenizer = None
    lm = SimpleNamespace(config=SimpleNamespace(vocab_size=TINY_V))


def test_refused_arguments():
    emb, neg = torch.zeros(2, 3, 8), torch.zeros(2, 4, 8)
    bad = [dict(guidance_scale=-0.5, negative_embeddings=neg), dict(guidance_scale=float("nan"), negative_embeddings=neg),
           dict(guidance_scale=float("inf"), negative_embeddings=neg), dict(guidance_scale=True, negative_embeddings=neg),
           dict(guidance_scale=2.0, negative_embeddings=neg, guidance_min_p=1.01),
           dict(guidance_scale=2.0, negative_embeddings=neg, guidance_min_p=-0.01),
           dict(guidance_scale=2.0),                                            # a scale without a negative prompt
           dict(negative_embeddings=neg), dict(guidance_scale=1.0, negative_embeddings=neg),      # a negative prompt at scale 1
           dict(guidance_min_p=0.1), dict(negative_lengths=[1, 2]),
           dict(guidance_scale=2.0, negative_embeddings=torch.zeros(3, 4, 8)),  # rows
           dict(guidance_scale=2.0, negative_embeddings=[torch.zeros(4, 8)] * 3),
           dict(guidance_scale=2.0, negative_embeddings=torch.zeros(2, 4, 16)),  # hidden size
           dict(guidance_scale=2.0, negative_embeddings=neg, negative_lengths=[1, 5]),
           dict(guidance_scale=2.0, negative_embeddings=neg, negative_lengths=[1]),
           dict(guidance_scale=2.0, negative_embeddings=(neg, torch.tensor([1, 2])), negative_lengths=[1, 2]),
           dict(guidance_scale=2.0, negative_embeddings=torch.zeros(4, 8))]
    for kw in bad:
        with pytest.raises(ValueError):
            generate(_NoModel(), emb, max_steps=2, **kw)
    for kw in (dict(num_beams=2), dict(return_scores=True), dict(past_key_values=object()), dict(return_past_key_values=True)):
        with pytest.raises(NotImplementedError):
            generate(_NoModel(), emb, max_steps=2, guidance_scale=2.0, negative_embeddings=neg, **kw)
    with pytest.raises(TypeError):          # keyword-only
        generate(_NoModel(), emb, 2, 0.0, 0, 0.9, EOS, False, True, None, None, None, 1, 1.0, False, 1, False, None, False, 2.0)
    # what is allowed, and what it is normalised to
    assert check_guidance_args() is None and check_guidance_args(1.0, None, None, 0.0, 2, 8) is None
    g = check_guidance_args(3, neg, None, 0.25, 2, 8)
    assert g["scale"] == 3.0 and g["min_p"] == 0.25 and g["embeddings"] is neg and g["lengths"] is None
    g = check_guidance_args(0.0, torch.ones(1, 4, 8), [3], 0.0, 2, 8)           # one row, broadcast
    assert g["embeddings"].shape == (2, 4, 8) and g["lengths"].tolist() == [3, 3]
    g = check_guidance_args(2.0, [torch.ones(4, 8), torch.ones(1, 2, 8)], None, 0.0, 2, 8)
    assert g["embeddings"].shape == (2, 4, 8) and g["lengths"].tolist() == [4, 2] and float(g["embeddings"][1, 2:].abs().sum()) == 0
    g = check_guidance_args(2.0, (neg, torch.tensor([4, 1])), None, 1.0, 2, 8)
    assert g["lengths"].tolist() == [4, 1] and g["min_p"] == 1.0


# ------------------------------------------------------------------------------------------ generate()'s host branch
N = 8


@pytest.fixture(scope="module")
def tiny():
    from test_logits_processors_cpu import _HostMagma
    model = _tiny_gptj(seed=4, eos_bias=1.5)
    g = torch.Generator().manual_seed(11)
    return _HostMagma(model), torch.randn(3, 5, 32, generator=g), torch.randn(3, 3, 32, generator=g)


def _two_streams(lm, emb, neg, scale, min_p, n, rules=None):
    """The loop written out: two model calls per step with two pasts, the statement cast to fp32, argmax."""
    from magma_amd.sampling import process_logits
    with torch.no_grad():
        oc, ou = lm(inputs_embeds=emb, use_cache=True), lm(inputs_embeds=neg, use_cache=True)
        hist = torch.zeros(emb.shape[0], n, dtype=torch.int64)
        for t in range(n):
            x = guide_logits(oc.logits[:, -1].float(), ou.logits[:, -1].float(), scale, min_p).to(torch.float32)
            if rules:
                x = process_logits(x, hist, t, eos_token=EOS, **rules)
            hist[:, t] = x.argmax(-1)
            oc = lm(input_ids=hist[:, t:t + 1], past_key_values=oc.past_key_values, use_cache=True)
            ou = lm(input_ids=hist[:, t:t + 1], past_key_values=ou.past_key_values, use_cache=True)
    return hist


def test_generate_host_branch_is_the_two_stream_loop(tiny):
    model, emb, neg = tiny
    S = emb.shape[1]
    kw = dict(max_steps=N, temperature=0.0, eos_token=EOS, decode=False, stop_on_eos=False)
    plain = generate(model, emb, **kw)
    assert torch.equal(generate(model, emb, guidance_scale=1.0, **kw), plain)       # 1.0 is the unguided call exactly
    differs = 0
    for scale, min_p in ((3.0, 0.0), (3.0, 0.1), (0.0, 0.0), (7.5, 0.5)):
        out = generate(model, emb, guidance_scale=scale, negative_embeddings=neg, guidance_min_p=min_p, **kw)
        assert out.shape == plain.shape and torch.equal(out[:, :S], plain[:, :S])     # the layout of the unguided call
        assert torch.equal(out[:, S:], _two_streams(model.lm.inner, emb, neg, scale, min_p, N)), (scale, min_p)
        differs += int(not torch.equal(out, plain))
    assert differs >= 2             # the guidance changed tokens
    # one negative row for every sample, and the rule in front of the repetition penalty
    one = generate(model, emb, guidance_scale=3.0, negative_embeddings=neg[:1], **kw)
    assert torch.equal(one[:, S:], _two_streams(model.lm.inner, emb, neg[:1].expand(3, -1, -1), 3.0, 0.0, N))
    rules = dict(repetition_penalty=1.7)
    pen = generate(model, emb, guidance_scale=3.0, negative_embeddings=neg, **rules, **kw)
    assert torch.equal(pen[:, S:], _two_streams(model.lm.inner, emb, neg, 3.0, 0.0, N, rules))
    # log-probabilities stay those of the raw conditional distribution
    from magma_amd.sampling import token_logprobs
    out, lps = generate(model, emb, guidance_scale=3.0, negative_embeddings=neg, return_logprobs=True, **kw)
    with torch.no_grad():
        o = model.lm.inner(inputs_embeds=emb, use_cache=True)
    want = token_logprobs(o.logits[:, -1].float(), out[:, S], 0)[0]
    assert torch.allclose(lps.logprobs[:, 0].double(), want, atol=1e-5, rtol=0)
    # ragged negative prompts need per-row KV positions: the host branch refuses them
    with pytest.raises(ValueError):
        generate(model, emb, guidance_scale=3.0, negative_embeddings=neg, negative_lengths=[3, 2, 1], **kw)
