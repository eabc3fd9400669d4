"""Regenerates STEP_QUANT_SHIFT of tests/test_w4a16_gpu.py: how far MXFP4 weight quantisation itself moves the logits of one
greedy token step, measured WITHOUT the kernels -- the fp32 CPU oracle on the dequantised weights against the same oracle on the
original weights, same inputs, same prefill cache (2 blocks, full width, B = 8, 16-token prefill, seed 97).  CPU only, about a
minute per config.

  python tools/w4_step_quant_shift.py"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fullwidth_common as F  # noqa: E402
from test_w4a16_gpu import STEP_CASES, TINY_TRUNK, no_ln_bias, rel  # noqa: E402

BF16 = torch.bfloat16


def cpu_dequantised_lm(lm, cfg):
    """The oracle's LM parameters with every decode operand replaced by what W4A16 multiplies by -- quantised as the engine does
    it (bf16 weights; ln_1 / ln_f gamma folded in before the quantiser, divided out after), entirely on the CPU."""
    from magma_amd import ops
    from oracle.model import attn_prefix, mlp_adapter_prefix, mlp_prefix
    dq = lambda w: ops.dequantize_mx_fp4(*ops.quantize_mx_fp4(w.to(BF16)))  # noqa: E731

    def folded(w, gamma):
        return dq((w.to(BF16).float() * gamma[None, :]).to(BF16)) / gamma[None, :]

    q, d = dict(lm), cfg.d_model
    for i in range(cfg.n_layer):
        ap, mp = attn_prefix(cfg, i), mlp_prefix(cfg, i)
        gam = lm[f"lm.transformer.h.{i}.ln_1.weight"]
        for name in (ap + "q_proj.weight", ap + "k_proj.weight", ap + "v_proj.weight", mp + "c_fc.weight"):
            q[name] = folded(lm[name], gam)
        names = [ap + "out_proj.weight", mp + "c_proj.weight"]
        if cfg.mlp_adapter_hidden:
            names += [mlp_adapter_prefix(cfg, i) + "0.weight", mlp_adapter_prefix(cfg, i) + "2.weight"]
        if cfg.attn_adapter_hidden:
            names += [f"lm.transformer.h.{i}.attn.adapter.0.weight", f"lm.transformer.h.{i}.attn.adapter.2.weight"]
        for name in names:
            q[name] = dq(lm[name])
    q["lm.lm_head.weight"] = folded(lm["lm.lm_head.weight"], lm["lm.transformer.ln_f.weight"])
    return q


if __name__ == "__main__":
    from oracle.model import lm_forward
    for name, (ckw, _) in STEP_CASES.items():
        t = time.time()
        cfg = F.full_width_config(n_layer=2, **ckw, **TINY_TRUNK)
        lm = F.lm_only(no_ln_bias(F.full_width_params(cfg)))
        emb = F.greedy_inputs(cfg, seed=97, B=8, S0=16)
        with torch.no_grad():
            r0 = lm_forward(lm, cfg, inputs_embeds=emb)
            tok = r0["logits"][:, -1].argmax(-1, keepdim=True)
            a = lm_forward(lm, cfg, input_ids=tok, past=r0["past_key_values"])["logits"][:, -1]
            b = lm_forward(cpu_dequantised_lm(lm, cfg), cfg, input_ids=tok, past=r0["past_key_values"])["logits"][:, -1]
        print(f"{name}: rel-L2(oracle on dequantised weights, oracle on original weights) = {rel(b, a):.4f}  ({time.time() - t:.0f} s)", flush=True)
