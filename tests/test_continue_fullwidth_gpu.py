"""Continuing from a KV cache at BASELINE WIDTH (d 4096, 16 heads, ff 16384, V 50 258; one GPT-J block,
tests/fullwidth_common.py): a right-padded batch of 8 prompts with lengths between 20 and 57 is prefilled, a ragged chunk of
9 to 40 rows per row is appended (LMEngine.extend: per-row rotary + KV append, mg_attn_prefill_cached_bf16), then 8 teacher-forced
cached steps.  Every row against the fp32 CPU oracle run on that row ALONE (lm_forward(inputs_embeds=chunk, past=prefix cache)).

Tolerance: the suite's rule -- err(HIP bf16, oracle fp32) <= 2 x err(oracle in bf16 on PyTorch CPU, oracle fp32) + floor
(rel-L2) per row and step, for the chunk's last row, every row of the chunk and the steps after it; greedy ids equal wherever
the oracle's top-2 margin exceeds TEST_MARGIN x std(logits), and at least 75 % of the decisions are such safe ones."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fullwidth_common as F  # noqa: E402

pytestmark = pytest.mark.gpu

PREFIX = [20, 57, 33, 41, 26, 50, 29, 45]
CHUNK = [9, 40, 17, 31, 12, 25, 36, 20]
STEPS = 8


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def test_continued_rows_match_the_oracle_alone(dev):
    from magma_amd.testing import build_reduced_magma
    from oracle.model import lm_forward
    cfg = F.full_width_config()
    lm = F.lm_only(F.full_width_params(cfg))
    lmb = {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in lm.items()}
    model = build_reduced_magma(dev, n_layer=1, n_head=16, d_ff=16384, vocab=50258, n_positions=2048)
    _, unexpected = model.load_checkpoint_state(lm)
    assert not unexpected
    model.eval()
    B, S, T = len(PREFIX), max(PREFIX), max(CHUNK)
    emb = F.greedy_inputs(cfg, seed=1357, B=B, S0=S + T)
    pre = torch.zeros(B, S, cfg.d_model)
    chunk = torch.zeros(B, T, cfg.d_model)
    for b, (n, c) in enumerate(zip(PREFIX, CHUNK)):
        pre[b, :n] = emb[b, :n]
        chunk[b, :c] = emb[b, n:n + c]
    # oracle, row by row: prefix -> cache, the chunk against that cache, then teacher-forced greedy steps
    refs, refs_b, full_ref, full_refb, feeds = [], [], [], [], []
    with torch.no_grad():
        for b, (n, c) in enumerate(zip(PREFIX, CHUNK)):
            r = lm_forward(lm, cfg, inputs_embeds=pre[b:b + 1, :n])
            rb = lm_forward(lmb, cfg, inputs_embeds=pre[b:b + 1, :n].to(torch.bfloat16))
            r = lm_forward(lm, cfg, inputs_embeds=chunk[b:b + 1, :c], past=r["past_key_values"])
            rb = lm_forward(lmb, cfg, inputs_embeds=chunk[b:b + 1, :c].to(torch.bfloat16), past=rb["past_key_values"])
            full_ref.append(r["logits"][0].float())
            full_refb.append(rb["logits"][0].float())
            lg, lgb, ids = [r["logits"][0, -1].float()], [rb["logits"][0, -1].float()], []
            past, pastb = r["past_key_values"], rb["past_key_values"]
            for _ in range(STEPS):
                tok = lg[-1].argmax().view(1, 1)
                ids.append(int(tok))
                r = lm_forward(lm, cfg, input_ids=tok, past=past)
                rb = lm_forward(lmb, cfg, input_ids=tok, past=pastb)
                past, pastb = r["past_key_values"], rb["past_key_values"]
                lg.append(r["logits"][0, -1].float())
                lgb.append(rb["logits"][0, -1].float())
            refs.append(lg)
            refs_b.append(lgb)
            feeds.append(ids)
        # HIP: ragged prefill, the ragged chunk appended to its cache, STEPS cached steps on the oracle's ids
        out = model.lm(inputs_embeds=pre.to(torch.bfloat16).to(dev), use_cache=True, cache_hint=4, lengths=PREFIX)
        cache = out.past_key_values
        smax0 = cache.Smax
        ext = model.lm(inputs_embeds=chunk.to(torch.bfloat16).to(dev), past_key_values=cache, use_cache=True, cache_hint=STEPS,
                       lengths=CHUNK)
        assert ext.past_key_values is cache and cache.Smax > smax0          # 57 + 40 + 8 rows outgrow the first cache
        assert cache.d_pos.tolist() == [n + c for n, c in zip(PREFIX, CHUNK)]
        got = [ext.logits[:, -1].float().cpu()]
        full = ext.full_logits.float().cpu()
        for i in range(STEPS):
            tok = torch.tensor([[feeds[b][i]] for b in range(B)], device=dev)
            o = model.lm(input_ids=tok, use_cache=True, past_key_values=cache)
            got.append(o.logits[:, -1].float().cpu().clone())
    assert cache.d_pos.tolist() == [n + c + STEPS for n, c in zip(PREFIX, CHUNK)]
    for b, c in enumerate(CHUNK):
        e, eb = rel(full[b, :c], full_ref[b]), rel(full_refb[b], full_ref[b])
        assert e <= 2.0 * eb + 2e-3, f"row {b}: chunk logits, HIP err {e:.3e} vs eager-bf16 err {eb:.3e}"
    n_safe = 0
    for i in range(STEPS + 1):
        for b in range(B):
            ref, refb, g = refs[b][i], refs_b[b][i], got[i][b]
            e, eb = rel(g, ref), rel(refb, ref)
            assert e <= 2.0 * eb + 2e-3, f"row {b} step {i}: HIP err {e:.3e} vs eager-bf16 err {eb:.3e}"
            top2 = torch.topk(ref, 2).values
            if float(top2[0] - top2[1]) > F.TEST_MARGIN * float(ref.std()):
                n_safe += 1
                assert int(g.argmax()) == int(ref.argmax()), f"row {b} step {i}: greedy id"
    assert n_safe >= 0.75 * B * (STEPS + 1), n_safe
