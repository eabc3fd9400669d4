"""Per-request sampling on the host (DESIGN.md "Per-request sampling"): the host statement of generate_stream(per_request=True) -- one
solo generate() per request with the request's OWN settings and seed, None fields taking the session's --, the argument checks of
the per-row generate() and of StreamRequest, the records check_row_sampler_args builds, the table's host image and the header."""
import os
import re
import struct

import pytest
import torch

from magma_amd import sampling
from magma_amd.sampling import StreamRequest, check_row_sampler_args, generate, generate_stream, per_row_given
from test_beam_search_cpu import EOS, V, _tiny_gptj
from test_logits_processors_cpu import _HostMagma
from test_stream_cpu import _NoModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_loop_passes_every_requests_own_settings_to_its_solo_call(monkeypatch):
    model = _HostMagma(_tiny_gptj(seed=4, eos_bias=1.5))
    g = torch.Generator().manual_seed(11)
    p = [torch.randn(n, 32, generator=g) for n in (5, 1, 7, 3, 4)]
    items = [StreamRequest(p[0], 3, temperature=0.0),                               # greedy beside sampled requests
             StreamRequest(p[1][None], temperature=1.1, top_k=5, top_p=0.5, min_p=0.1, seed=41),
             (p[2], 2),                                                             # a pair: the session's settings and seed
             StreamRequest(p[3], seed=43),                                          # only the seed is its own
             p[4]]
    seen = []
    solo = sampling.generate

    def spy(m, emb, **kw):
        seen.append(kw)
        return solo(m, emb, **kw)

    monkeypatch.setattr(sampling, "generate", spy)
    torch.manual_seed(0)
    got = list(generate_stream(model, items, max_new_tokens=6, max_prompt=8, decode=False, per_request=True, sampler="transformers",
                               temperature=0.7, top_k=9, top_p=0.8, min_p=0.0, seed=7))
    assert [r.index for r in got] == [0, 1, 2, 3, 4] and all(r.slot is None for r in got)
    want = [dict(temperature=0.0, top_k=9, top_p=0.8, min_p=0.0, seed=0, max_steps=3),           # a greedy request reads no seed
            dict(temperature=1.1, top_k=5, top_p=0.5, min_p=0.1, seed=41, max_steps=6),
            dict(temperature=0.7, top_k=9, top_p=0.8, min_p=0.0, seed=7, max_steps=2),
            dict(temperature=0.7, top_k=9, top_p=0.8, min_p=0.0, seed=43, max_steps=6),
            dict(temperature=0.7, top_k=9, top_p=0.8, min_p=0.0, seed=7, max_steps=6)]
    assert len(seen) == 5
    for kw, w in zip(seen, want):
        assert {k: kw[k] for k in w} == w and kw["sampler"] == "transformers" and kw["stop_per_row"] is True
    # the greedy request is the plain greedy solo call
    out, fin = solo(model, p[0][None], max_steps=3, temperature=0.0, stop_per_row=True, return_finish=True, decode=False, eos_token=[EOS])
    assert got[0].tokens.tolist() == out[0, 5: 5 + int(fin.kept[0])].tolist()
    # a sampled request without a seed of its own or of the session draws one from torch's CPU generator when it is pulled
    seen.clear()
    torch.manual_seed(5)
    list(generate_stream(model, [StreamRequest(p[3], 2, temperature=0.9)], max_new_tokens=2, max_prompt=8, decode=False, per_request=True))
    torch.manual_seed(5)
    assert seen[0]["seed"] == int(torch.randint(0, 2 ** 62, (1,)).item())


def test_stream_request_checks():
    model = _HostMagma(_tiny_gptj(seed=4, eos_bias=1.5))
    ok = torch.randn(3, 32, generator=torch.Generator().manual_seed(1))
    kw = dict(max_new_tokens=4, max_prompt=8, decode=False)
    it = generate_stream(model, [ok, StreamRequest(ok)], **kw)                      # a StreamRequest without per_request=True
    assert next(it).index == 0
    with pytest.raises(ValueError, match="request 1: a StreamRequest needs generate_stream\\(..., per_request=True\\)"):
        next(it)
    for bad, what in [(StreamRequest(ok, min_p=0.1, temperature=0.7), "request 1: min_p needs sampler"),
                      (StreamRequest(ok, temperature=-0.5), "request 1: temperature"),
                      (StreamRequest(ok, temperature=float("nan")), "request 1: temperature"),
                      (StreamRequest(ok, top_k=-1), "request 1: top_k"), (StreamRequest(ok, top_p=1.5), "request 1: top_p"),
                      (StreamRequest(ok, seed=1.5), "request 1: seed"), (StreamRequest(ok, 5), "request 1: max_new_tokens"),
                      (StreamRequest(torch.randn(9, 32)), "request 1: a prompt of 9 rows"), (StreamRequest("text"), "request 1")]:
        it = generate_stream(model, [ok, bad], per_request=True, **kw)
        assert next(it).index == 0
        with pytest.raises(ValueError, match=what):
            next(it)
    it = generate_stream(model, [StreamRequest(ok, temperature=0.0, min_p=0.1)], per_request=True, sampler="transformers", **kw)
    with pytest.raises(ValueError, match="request 0: min_p applies to sampled selection"):
        next(it)
    # the session's own keywords are checked when the call is made; the refused keywords stay refused
    for session_kw in (dict(per_request=1), dict(per_request=True, seed=1.5), dict(per_request=True, min_p=0.5),
                       dict(per_request=True, sampler="other")):
        with pytest.raises(ValueError):
            generate_stream(_NoModel(), [ok], **session_kw)
    for refused in (dict(num_beams=2), dict(penalty_alpha=0.6), dict(guidance_scale=1.5), dict(repetition_penalty=1.3)):
        with pytest.raises(NotImplementedError, match="not combined with generate_stream yet"):
            generate_stream(_NoModel(), [ok], per_request=True, **refused)
    assert "temperature=0.5" in repr(StreamRequest(ok, temperature=0.5)) and "top_k" not in repr(StreamRequest(ok, temperature=0.5))


def test_per_row_generate_argument_checks():
    model = _HostMagma(_tiny_gptj(seed=4, eos_bias=1.5))
    emb = torch.randn(3, 4, 32, generator=torch.Generator().manual_seed(2))
    kw = dict(max_steps=2, decode=False)
    for given, what in [(dict(seed=[1, 2]), "seed has 2 entries, the batch 3 rows"),
                        (dict(temperature=torch.tensor([0.7, 0.7, 0.7, 0.7])), "temperature has 4 entries"),
                        (dict(min_p=[0.0, 0.1, 0.0]), "row 1: min_p needs sampler=\"transformers\""),
                        (dict(min_p=0.1, temperature=[0.7, 0.7, 0.7]), "min_p needs sampler=\"transformers\""),
                        (dict(min_p=[0.1, 0.1, 0.1], temperature=[0.7, 0.7, 0.0], sampler="transformers"),
                         "row 2: min_p applies to sampled selection"),
                        (dict(top_p=[0.9, 1.5, 0.9]), "row 1: top_p"), (dict(top_p=[0.9, 0.9, -0.1], sampler="transformers"), "row 2: "),
                        (dict(top_k=[0, 0, -1]), "row 2: top_k"), (dict(top_k=[0, 1.5, 0]), "row 1: top_k"),
                        (dict(temperature=[0.7, float("inf"), 0.7]), "row 1: temperature"), (dict(seed=[1, "a", 3]), "row 1: seed"),
                        (dict(seed=(1, 2, 3)), "need the HIP engine's LM")]:      # every check passed: the host loop has no per-row launch
        with pytest.raises(ValueError, match=what):
            generate(model, emb, **{**kw, **given})
    for bad in (dict(num_beams=2), dict(return_scores=True), dict(penalty_alpha=0.6, top_k=4),
                dict(guidance_scale=2.0, negative_embeddings=emb), dict(num_beams=4, num_beam_groups=2, diversity_penalty=0.5)):
        with pytest.raises(NotImplementedError, match="per-row sampler settings \\(seed given per row\\) are not combined with"):
            generate(model, emb, seed=[1, 2, 3], **{**kw, **bad})
    assert per_row_given(temperature=0.7, top_k=0, top_p=0.9, min_p=0.0, seed=None) == ()
    assert per_row_given(temperature=torch.tensor(0.7), seed=5) == ()                # a 0-dimensional tensor is a scalar
    assert per_row_given(temperature=[0.7], top_k=(1,), seed=torch.tensor([3])) == ("temperature", "top_k", "seed")


def test_records_and_the_tables_host_image():
    from magma_amd import ops
    torch.manual_seed(3)
    recs = check_row_sampler_args(4, "transformers", [0.0, 0.7, 1.3, 0.7], 40, torch.tensor([0.9, 0.5, 1.0, 0.0], dtype=torch.float64),
                                  [0.0, 0.1, 0.0, 0.0],
                                  [9, None, 2 ** 63 + 5, 8])
    torch.manual_seed(3)
    drawn = int(torch.randint(0, 2 ** 62, (1,)).item())
    assert recs[0] == (0.0, 40, 0.9, 0.0, 0)                          # a greedy row reads no seed
    assert recs[1][:4] == (0.7, 40, 0.5, 0.1) and recs[1][4] == drawn  # a sampled row without one draws it where the scalar call does
    assert recs[2][4] == 5 and recs[3][4] == 8                        # masked to 63 bits, as the scalar seed is
    table = ops.sample_rows_table(*zip(*recs))
    assert table.dtype == torch.uint8 and tuple(table.shape) == (4, ops.SAMPLE_ROW_BYTES) and ops.SAMPLE_ROW_BYTES == 32
    import math
    for r, (t, k, p, m, sd) in enumerate(recs):
        top_p, log_min_p, seed, temp, top_k = struct.unpack("<ddQfi", bytes(table[r].tolist()))
        assert (top_p, seed, top_k) == (p, sd, k) and temp == struct.unpack("<f", struct.pack("<f", t))[0]
        assert log_min_p == (math.log(m) if m > 0 else -math.inf)


def test_selection_plan_rows_mode():
    from magma_amd.selection import TokenSelection
    stop = dict(eos_ids=[EOS])
    plan = TokenSelection.selection_plan(sampling=("rows", True), stop=stop, vocab=V, slots=True)
    assert plan.mode == ("rows", True) and plan.is_rows and plan.slots and plan.graph_key(True).mode == ("rows", True)
    assert not TokenSelection.selection_plan(sampling=(0.7, 40, 0.9), vocab=V).is_rows
    assert TokenSelection.selection_plan(sampling=("rows", 0), vocab=V).mode == ("rows", False)
    with pytest.raises(ValueError):
        TokenSelection.selection_plan(sampling=("rows",), vocab=V)
    for kw in (dict(beam=(2, 1.0, False, 8)), dict(guidance=(1.5, 0.0)), dict(contrast=(4, 0.6))):
        with pytest.raises(NotImplementedError):
            TokenSelection.selection_plan(sampling=("rows", False), vocab=V, **kw)


def test_header_declares_the_entry_point_at_abi_27():
    from magma_amd import lib
    header = open(os.path.join(ROOT, "include", "magma_hip.h")).read()
    assert "#define MG_ABI_VERSION 27" in header and lib.ABI_VERSION == 27
    assert "#define MG_SAMPLE_ROW_BYTES 32" in header
    assert re.search(r"\bint mg_sample_rows_f32\(const float\* logits, int64_t ld, int32_t R, int32_t V, int32_t warp, const void\* params,",
                     header)
    declared = set(re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", header)) - {"mg_epilogue", "mg_gemm_desc", "mg_skinny_desc"}
    assert "mg_sample_rows_f32" in declared and declared == set(lib.SYMBOLS)
    if lib.LIB_PATH.exists():           # exported symbols equal declared ones (a build without the library checks the binding alone)
        import ctypes
        try:
            dll = ctypes.CDLL(str(lib.LIB_PATH))
        except OSError:
            return
        assert all(hasattr(dll, name) for name in declared)
