"""A SHARED session prefix at full width (share_prefix=True; d 4096, 16 heads, ff 16384, V 50258, one block; the model, requests,
seeds and thresholds of tests/test_stream_prefix_fullwidth_gpu.py): five requests through a slot session of two slots behind ONE
copy of a 37-row prefix that the prefix-partials launch reads for both rows, every id compared
with the fp32 CPU oracle's free-running greedy decode of cat([prefix, request]) ALONE, by the rule and ORACLE_MARGIN of
tests/test_continue_generate_gpu.py -- ids are compared up to the first decision within the margin.

The request seeds were chosen on the CPU with the oracle alone (per request the first seed of 100 i + 1, 100 i + 2, ... whose
decisions behind the prefix all have a top-1 / top-2 gap above 0.08 std(logits)), so that at least 80 % of all generated tokens
are compared."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fullwidth_common as F  # noqa: E402
from test_continue_generate_gpu import ORACLE_MARGIN  # noqa: E402

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
P, PREFIX_SEED = 37, 7
LENS, LIMITS, SEEDS = [57, 3, 20, 64, 9], [6, 10, 4, 8, 10], [7, 112, 206, 336, 429]


def test_five_requests_two_slots_behind_a_shared_prefix_equal_the_oracle_alone(dev, monkeypatch):
    from magma_amd.sampling import generate_stream
    from magma_amd.testing import build_reduced_magma
    from oracle.model import generate_greedy
    cfg = F.full_width_config(enc_width=16, enc_layers=(1, 1, 2, 1))
    params = F.full_width_params(cfg)
    model = build_reduced_magma(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=cfg.n_positions, enc_width=16,
                                enc_layers=(1, 1, 2, 1))
    missing, unexpected = model.load_checkpoint_state(params)
    assert not unexpected and not missing, (missing[:4], unexpected[:4])
    model.eval()
    lm = F.lm_only(params)
    prefix = torch.randn(P, cfg.d_model, generator=torch.Generator().manual_seed(PREFIX_SEED)).to(BF16)
    prompts = [torch.randn(n, cfg.d_model, generator=torch.Generator().manual_seed(s)).to(BF16) for n, s in zip(LENS, SEEDS)]
    eos = 50257
    from magma_amd import ops
    launches = {"prefix": 0, "shared": 0, "unshared": 0}
    for name in ("attn_decode_prefix", "decode_attn_gemv", "attn_decode_fused"):
        def spy(*a, _fn=getattr(ops, name), _name=name, **kw):
            launches["prefix" if _name == "attn_decode_prefix" else "shared" if kw.get("shared") is not None else "unshared"] += 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    got = list(generate_stream(model, [(p.to(dev), n) for p, n in zip(prompts, LIMITS)], slots=2, every=3, max_new_tokens=max(LIMITS),
                               max_prompt=64, eos_token=[eos], decode=False, prefix=prefix.to(dev), share_prefix=True))
    assert sorted(r.index for r in got) == list(range(5)) and {r.slot for r in got} == {0, 1}
    # the token steps ran the new launches (eager steps and captures are seen here, replays are not), never the unshared attention
    assert launches["prefix"] == launches["shared"] >= 1 and launches["unshared"] == 0, launches
    compared = total = 0
    for r in sorted(got, key=lambda r: r.index):
        ids, limit = r.tokens.tolist(), LIMITS[r.index]
        conv = torch.cat([prefix, prompts[r.index]]).float()[None]
        with torch.no_grad():
            toks, logits = generate_greedy(lm, cfg, conv, limit, stop_on_eos=False)
        ref = toks[0, P + LENS[r.index]:].tolist()
        assert 1 <= len(ids) <= limit and (len(ids) == limit or ids[-1] == eos), (r, ref)
        assert r.reason == ("eos" if ids[-1] == eos else "length")
        total += len(ids)
        for i, x in enumerate(ids):
            top2 = torch.topk(logits[i][0], 2).values
            if float(top2[0] - top2[1]) <= ORACLE_MARGIN * float(logits[i][0].std()):
                break
            assert x == ref[i], f"request {r.index}, token {i}: engine {x} != oracle {ref[i]} (engine {ids}, oracle {ref})"
            compared += 1
    print(f"compared {compared} of {total} generated tokens ({compared / total:.0%})")
    assert compared >= 0.8 * total, (compared, total)
