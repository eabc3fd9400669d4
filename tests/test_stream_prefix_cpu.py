"""A session prefix on the host (DESIGN.md "Request streams", session prefix): generate_stream(prefix=p) over the tiny random GPT-J
of tests/test_stream_cpu.py runs the solo generate() on cat([p, request_i]) per request; the argument checks of ``prefix`` and the
budgets with it; prefix=None and the refusals are what they were.  No GPU: the admission kernel is tested in
tests/test_stream_prefix_kernels_gpu.py, the engine's session in tests/test_stream_prefix_gpu.py."""
import pytest
import torch

from magma_amd.sampling import generate, generate_stream
from test_beam_search_cpu import EOS, V, _tiny_gptj
from test_logits_processors_cpu import _HostMagma
from test_stream_cpu import _NoModel


@pytest.fixture(scope="module")
def tiny():
    return _HostMagma(_tiny_gptj(seed=4, eos_bias=1.5))


def test_host_loop_runs_the_solo_call_on_the_concatenation(tiny):
    g = torch.Generator().manual_seed(14)
    lens, limits = [5, 1, 7, 3, 5, 2], [12, 1, 3, 12, 6, None]
    prefix = torch.randn(9, 32, generator=g)
    prompts = [torch.randn(1, n, 32, generator=g) if i % 2 else torch.randn(n, 32, generator=g) for i, n in enumerate(lens)]
    convs = [torch.cat([prefix, p.view(-1, 32)])[None] for p in prompts]
    plain = [generate(tiny, c, max_steps=12, temperature=0.0, eos_token=EOS, decode=False, stop_on_eos=False)[0, c.shape[1]:].tolist()
             for c in convs]
    eos_ids, caps = [EOS, V - 3], [n or 12 for n in limits]

    def reason(row, cap, seq):
        for t in range(cap):
            if row[t] in eos_ids:
                return "eos"
            if t >= 1 and row[t - 1: t + 1] == seq:
                return "stop"
        return "length"

    # a request's own two tokens under which the six requests end in all three ways
    seq = next(row[t:t + 2] for row in plain for t in range(1, 11)
               if {reason(r, c, row[t:t + 2]) for r, c in zip(plain, caps)} == {"eos", "stop", "length"})
    kw = dict(eos_token=[EOS, V - 3], stop_sequences=[seq])
    for given in (prefix, prefix[None]):
        got = list(generate_stream(tiny, [p if n is None else (p, n) for p, n in zip(prompts, limits)], max_new_tokens=12, max_prompt=8,
                                   decode=False, prefix=given, **kw))
        assert [r.index for r in got] == list(range(len(prompts)))
        reasons = set()
        for r, c, limit in zip(got, convs, limits):
            out, fin = generate(tiny, c, max_steps=limit or 12, stop_per_row=True, return_finish=True, temperature=0.0, decode=False, **kw)
            assert r.tokens.tolist() == out[0, c.shape[1]: c.shape[1] + int(fin.kept[0])].tolist() and 1 <= len(r.tokens) <= (limit or 12)
            assert (r.reason, r.reason_index, r.text, r.slot) == (fin.reason[0], fin.index[0], None, None)
            reasons.add(r.reason)
        assert reasons == {"eos", "stop", "length"}, [(r.reason, r.tokens.tolist()) for r in got]
    # the prefix is part of what the model reads: without it the ids are others
    bare = list(generate_stream(tiny, list(zip(prompts, [n or 12 for n in limits])), max_new_tokens=12, max_prompt=8, decode=False, **kw))
    assert [r.tokens.tolist() for r in bare] != [r.tokens.tolist() for r in got]


def test_prefix_argument_checks(tiny):
    reqs = [torch.zeros(2, 32)]
    ok = torch.zeros(9, 32)
    for bad in [torch.zeros(9, 31), torch.zeros(1, 9, 33), torch.zeros(2, 9, 32), torch.zeros(32), torch.zeros(0, 32), "text", 3]:
        with pytest.raises(ValueError, match="prefix"):
            generate_stream(tiny, reqs, max_new_tokens=4, max_prompt=8, prefix=bad)
    # the budgets: n_positions = 64 for the tiny model
    generate_stream(tiny, reqs, max_new_tokens=4, max_prompt=51, prefix=ok)
    with pytest.raises(ValueError, match="a prefix of 9 rows"):
        generate_stream(tiny, reqs, max_new_tokens=4, max_prompt=52, prefix=ok)
    generate_stream(tiny, reqs, max_new_tokens=4, max_prompt=52)                  # ... which fits without the prefix
    with pytest.raises(ValueError, match="no room"):
        generate_stream(tiny, reqs, max_new_tokens=50, prefix=ok)                 # (64 - 9 - 50) // 64 * 64 = 0
    with pytest.raises(ValueError, match="a prefix of 100 rows"):
        generate_stream(_NoModel(), reqs, max_new_tokens=57, max_prompt=100, prefix=torch.zeros(100, 8))      # 257 > 256


def test_default_max_prompt_counts_the_prefix():
    """max_position_embeddings = 256: the default is (256 - P - max_new_tokens) // 64 * 64, the longest request NOT counting the
    prefix -- read off the error a request one row longer raises when it is pulled."""
    for P, max_new, want in [(0, 20, 192), (37, 20, 192), (44, 20, 192), (45, 20, 128), (100, 28, 128), (1, 191, 64)]:
        prefix = torch.zeros(P, 8) if P else None
        it = generate_stream(_NoModel(), [torch.zeros(want + 1, 8)], max_new_tokens=max_new, prefix=prefix, decode=False)
        with pytest.raises(ValueError, match=rf"request 0: a prompt of {want + 1} rows is outside \[1, max_prompt = {want}\]"):
            next(it)


def test_a_cache_prefix_needs_the_engine(tiny):
    from magma_amd.engine import KVCache
    cache = KVCache(1, 1, 1, 64, "cpu")
    with pytest.raises(ValueError, match="KVCache prefix needs the HIP engine"):
        generate_stream(tiny, [torch.zeros(2, 32)], max_new_tokens=4, max_prompt=8, prefix=cache)


def test_no_prefix_and_the_refusals_are_what_they_were(tiny):
    g = torch.Generator().manual_seed(11)
    prompts = [torch.randn(n, 32, generator=g) for n in (5, 1, 7)]
    kw = dict(max_new_tokens=6, max_prompt=8, eos_token=[EOS, V - 3], decode=False)
    a = list(generate_stream(tiny, prompts, **kw))
    b = list(generate_stream(tiny, prompts, prefix=None, **kw))
    assert [(r.index, r.tokens.tolist(), r.reason, r.reason_index, r.slot) for r in a] == \
        [(r.index, r.tokens.tolist(), r.reason, r.reason_index, r.slot) for r in b]
    for r, p in zip(a, prompts):
        out, fin = generate(tiny, p[None], max_steps=6, eos_token=[EOS, V - 3], stop_per_row=True, return_finish=True, temperature=0.0,
                            decode=False)
        assert r.tokens.tolist() == out[0, p.shape[0]: p.shape[0] + int(fin.kept[0])].tolist() and r.reason == fin.reason[0]
    for bad in [dict(past_key_values=object()), dict(return_past_key_values=True)]:
        with pytest.raises(NotImplementedError, match=r"a KV cache \(past_key_values / return_past_key_values\) is not combined with "
                                                      "generate_stream yet"):
            generate_stream(tiny, prompts, prefix=torch.zeros(3, 32), **kw, **bad)
    with pytest.raises(TypeError):          # keyword-only, like every other argument
        generate_stream(tiny, prompts, 8, 6, 8, None, None, 0.0, 0, 0.9, "reference", 0.0, None, None, None, False, torch.zeros(3, 32))
