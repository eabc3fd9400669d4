"""share_prefix on the host (DESIGN.md "Shared session prefix"): the argument checks of generate_stream(share_prefix=...), an LM
object that is not the HIP engine ignores the flag -- the host loop runs the solo calls on cat([prefix, request_i]) either way --,
the budget arithmetic is what it was, and the chunking the kernels use is a function of P alone.  No GPU: the kernels are tested in
tests/test_shared_prefix_kernels_gpu.py, the engine's session in tests/test_stream_shared_prefix_gpu.py."""
import inspect
import os

import pytest
import torch

from magma_amd.sampling import generate_stream
from test_beam_search_cpu import EOS, V, _tiny_gptj
from test_logits_processors_cpu import _HostMagma
from test_stream_cpu import _NoModel


@pytest.fixture(scope="module")
def tiny():
    return _HostMagma(_tiny_gptj(seed=4, eos_bias=1.5))


def test_share_prefix_argument_checks(tiny):
    reqs = [torch.zeros(2, 32)]
    assert inspect.signature(generate_stream).parameters["share_prefix"].default is False
    for model, width in ((tiny, 32), (_NoModel(), 8)):
        with pytest.raises(ValueError, match="share_prefix=True needs a prefix"):      # at call time: nothing is pulled
            generate_stream(model, iter(()), max_new_tokens=4, max_prompt=8, share_prefix=True)
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="share_prefix must be True or False"):
                generate_stream(model, reqs, max_new_tokens=4, max_prompt=8, prefix=torch.zeros(3, width), share_prefix=bad)
        generate_stream(model, reqs, max_new_tokens=4, max_prompt=8, prefix=torch.zeros(3, width), share_prefix=True)
        generate_stream(model, reqs, max_new_tokens=4, max_prompt=8, share_prefix=False)
    # every refusal of a stream stays, with the flag as without it
    for bad in (dict(repetition_penalty=1.3), dict(return_logprobs=True), dict(constraint=[[1, 2]]), dict(guidance_scale=1.5),
                dict(num_beams=2), dict(penalty_alpha=0.6), dict(past_key_values=object())):
        with pytest.raises(NotImplementedError, match="not combined with generate_stream yet"):
            generate_stream(tiny, reqs, max_new_tokens=4, max_prompt=8, prefix=torch.zeros(3, 32), share_prefix=True, **bad)


def test_the_host_loop_ignores_the_flag(tiny):
    g = torch.Generator().manual_seed(11)
    prompts = [torch.randn(n, 32, generator=g) for n in (5, 1, 7, 3, 5, 2)]
    prefix = torch.randn(9, 32, generator=g)
    kw = dict(max_new_tokens=8, max_prompt=8, eos_token=[EOS, V - 3], decode=False, prefix=prefix)
    a = list(generate_stream(tiny, prompts, share_prefix=False, **kw))
    b = list(generate_stream(tiny, prompts, share_prefix=True, **kw))
    assert len(a) == len(b) == len(prompts)
    for x, y in zip(a, b):
        assert (x.index, x.tokens.tolist(), x.reason, x.reason_index, x.slot) == (y.index, y.tokens.tolist(), y.reason, y.reason_index, y.slot)
    assert {r.reason for r in a} >= {"length"} and len({tuple(r.tokens.tolist()) for r in a}) > 1


def test_the_budget_is_unchanged():
    """P + max_prompt + max_new_tokens <= max_position_embeddings (256 here), shared or not; the default max_prompt counts P."""
    reqs = [torch.zeros(2, 8)]
    for share in (False, True):
        generate_stream(_NoModel(), reqs, max_new_tokens=56, max_prompt=100, prefix=torch.zeros(100, 8), share_prefix=share)      # 256
        with pytest.raises(ValueError, match="a prefix of 100 rows"):
            generate_stream(_NoModel(), reqs, max_new_tokens=57, max_prompt=100, prefix=torch.zeros(100, 8), share_prefix=share)  # 257
        it = generate_stream(_NoModel(), [torch.zeros(129, 8)], max_new_tokens=20, prefix=torch.zeros(100, 8), share_prefix=share,
                             decode=False)
        with pytest.raises(ValueError, match=r"max_prompt = 128\]"):      # (256 - 100 - 20) // 64 * 64
            next(it)


def test_the_chunking_depends_on_the_prefix_alone():
    from magma_amd import ops
    assert (ops.PREFIX_CHUNK, ops.PREFIX_PART) == (64, 264)
    assert [ops.prefix_chunks(p) for p in (1, 63, 64, 65, 128, 129, 656, 4096)] == [1, 1, 1, 2, 2, 3, 11, 64]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "magma_hip.h")).read()
    assert "#define MG_PREFIX_CHUNK 64" in header and "#define MG_PREFIX_PART 264" in header and "#define MG_ABI_VERSION 27" in header
