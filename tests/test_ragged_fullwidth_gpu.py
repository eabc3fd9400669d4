"""Ragged batches at BASELINE WIDTH (d 4096, 16 heads, ff 16384, V 50 258; one GPT-J block, tests/fullwidth_common.py): a
right-padded batch of 8 prompts with lengths between 20 and 57, prefill + 8 teacher-forced cached steps, every row against
the fp32 CPU oracle run on that row ALONE (unpadded, B = 1).

Tolerance: the suite's rule -- err(HIP bf16, oracle fp32) <= 2 x err(oracle in bf16 on PyTorch CPU, oracle fp32) + floor
(rel-L2) per row and step; greedy ids equal wherever the oracle's top-2 margin exceeds TEST_MARGIN x std(logits), and at
least 75 % of the decisions are such safe ones."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fullwidth_common as F  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [20, 57, 33, 41, 26, 50, 29, 45]
STEPS = 8


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def test_ragged_rows_match_the_oracle_alone(dev):
    from magma_amd.testing import build_reduced_magma
    from oracle.model import lm_forward
    cfg = F.full_width_config()
    lm = F.lm_only(F.full_width_params(cfg))
    lmb = {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in lm.items()}
    model = build_reduced_magma(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=2048)
    _, unexpected = model.load_checkpoint_state(lm)
    assert not unexpected
    model.eval()
    B, S = len(LENGTHS), max(LENGTHS)
    emb = F.greedy_inputs(cfg, seed=2468, B=B, S0=S)
    for b, n in enumerate(LENGTHS):
        emb[b, n:] = 0
    # teacher forcing: row b is fed the fp32 oracle's own greedy choices for that row alone
    refs, refs_b, feeds = [], [], []
    with torch.no_grad():
        for b, n in enumerate(LENGTHS):
            x = emb[b:b + 1, :n]
            r = lm_forward(lm, cfg, inputs_embeds=x)
            rb = lm_forward(lmb, cfg, inputs_embeds=x.to(torch.bfloat16))
            lg, lgb, ids = [r["logits"][0, -1]], [rb["logits"][0, -1].float()], []
            past, pastb = r["past_key_values"], rb["past_key_values"]
            for _ in range(STEPS):
                tok = lg[-1].argmax().view(1, 1)
                ids.append(int(tok))
                r = lm_forward(lm, cfg, input_ids=tok, past=past)
                rb = lm_forward(lmb, cfg, input_ids=tok, past=pastb)
                past, pastb = r["past_key_values"], rb["past_key_values"]
                lg.append(r["logits"][0, -1])
                lgb.append(rb["logits"][0, -1].float())
            refs.append(lg)
            refs_b.append(lgb)
            feeds.append(ids)
        out = model.lm(inputs_embeds=emb.to(torch.bfloat16).cuda(), use_cache=True, cache_hint=STEPS + 4, lengths=LENGTHS)
        cache = out.past_key_values
        got = [out.logits[:, -1].float().cpu()]
        for i in range(STEPS):
            tok = torch.tensor([[feeds[b][i]] for b in range(B)], device=dev)
            o = model.lm(input_ids=tok, use_cache=True, past_key_values=cache)
            got.append(o.logits[:, -1].float().cpu().clone())
    assert cache.d_pos.tolist() == [n + STEPS for n in LENGTHS]
    n_safe = 0
    for i in range(STEPS + 1):
        for b in range(B):
            ref, refb, g = refs[b][i], refs_b[b][i], got[i][b]
            e, eb = rel(g, ref), rel(refb, ref)
            assert e <= 2.0 * eb + 2e-3, f"row {b} (len {LENGTHS[b]}) step {i}: HIP err {e:.3e} vs eager-bf16 err {eb:.3e}"
            top2 = torch.topk(ref, 2).values
            if float(top2[0] - top2[1]) > F.TEST_MARGIN * float(ref.std()):
                n_safe += 1
                assert int(g.argmax()) == int(ref.argmax()), f"row {b} step {i}: greedy id"
    assert n_safe >= 0.75 * B * (STEPS + 1), n_safe
