"""Multi-turn generation: turn 2 continued from turn 1's KV cache against a fresh generate over the concatenated conversation,
the shared-prefix case (one cached prompt expanded to B questions) against B full prompts, and the chunk attention launch
(mg_attn_prefill_cached_bf16) alone.  MAGMA_v1, random weights, B = 8.

    python tools/continue_generate_bench.py [--layers 28] [--steps 5] [--warmup 2]

Turn 1: 144-row image prefix + 24 text rows, 32 greedy tokens.  Turn 2: a 16-token question, 32 greedy tokens.  The legs run
interleaved.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12          # MI355X peak HBM bandwidth: the floor of a launch that reads the K / V once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="MAGMA_v1")
    ap.add_argument("--layers", type=int, default=None, help="GPT-J blocks (default: the config's 28)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--gen", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    from magma_amd import Magma, ops
    from magma_amd.language_model import GPTJConfig
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    lm_cfg = GPTJConfig(num_layers=args.layers, vocab_size=50258) if args.layers else None
    model = Magma(args.config, device=dev, lm_config=lm_cfg)
    model.eval()
    B, gen, d = args.batch, args.gen, model.lm.config.hidden_size
    P, TXT, Q = 144, 24, 16
    g = torch.Generator(device=dev).manual_seed(7)
    prompt = (torch.randn(B, P + TXT, d, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    quest = (torch.randn(B, Q, d, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    eos = model.eos_token
    kw = dict(max_steps=gen, temperature=0.0, decode=False, stop_on_eos=False)

    out1, past1 = model.generate(prompt, return_past_key_values=True, **kw)
    wte = model.lm.engine.wte
    conv = []
    for b in range(B):
        t = out1[b, P + TXT:].tolist()
        t = t[: t.index(eos)] if eos in t else t
        conv.append(torch.cat([prompt[b], wte[torch.tensor(t, dtype=torch.long, device=dev)], quest[b]], 0))

    def timed(fn, setup=None):
        ts = []
        for i in range(args.warmup + args.steps):
            arg = setup() if setup else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(arg)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(time.perf_counter() - t0)
        return round(min(ts) * 1e3, 3)

    # the continued legs run on caller-held caches that keep their captured token steps (as a conversation does from turn to
    # turn); before every run the turn-1 / expanded state is copied back in, untimed (expand_copy_ms: what that copy costs)
    rows1, pend1 = past1.rows_pos(), past1.pending.clone()
    work = past1.expand(1)
    shared = model.cache_prompt(prompt[:1])
    work8 = shared.expand(B)
    rows8 = work8.rows_pos()

    def reset(dst, src, rows, pend):
        dst.k.copy_(src.k)
        dst.v.copy_(src.v)
        dst.set_rows(rows, pend)
        return dst

    ref8 = shared.expand(B)
    legs = {}
    for rep in range(2):                    # interleaved twice: drift of the box shows as a spread between the two rounds
        legs.setdefault("turn2_continued_ms", []).append(
            timed(lambda p: model.generate(quest, past_key_values=p, **kw), setup=lambda: reset(work, past1, rows1, pend1)))
        legs.setdefault("turn2_fresh_ms", []).append(timed(lambda _: model.generate(conv, **kw)))
        legs.setdefault("shared_prefix_expand_ms", []).append(
            timed(lambda p: model.generate(quest, past_key_values=p, **kw), setup=lambda: reset(work8, ref8, rows8, None)))
        legs.setdefault("expand_copy_ms", []).append(timed(lambda _: shared.expand(B)))
        legs.setdefault("shared_prefix_full_prompts_ms", []).append(
            timed(lambda _: model.generate(torch.cat([prompt[:1].expand(B, -1, -1), quest], 1), **kw)))
    best = {k: min(v) for k, v in legs.items()}

    # the chunk attention launch alone, next to the decode attention over the same cache and the K / V bytes-over-bandwidth floor
    H = model.lm.config.num_heads
    kern = []
    for p in (256, 1024):
        Smax = p + 128
        kc = torch.randn(B, H, Smax, 256, device=dev, generator=g).to(torch.bfloat16)
        vc = torch.randn(B, H, Smax, 256, device=dev, generator=g).to(torch.bfloat16)
        d_pos = torch.full((B,), p, dtype=torch.int32, device=dev)
        for T in (1, 16, 64, 128):
            q = torch.randn(B, H, T, 256, device=dev, generator=g).to(torch.bfloat16)
            o = torch.empty(B * T, H * 256, dtype=torch.bfloat16, device=dev)
            us = _launch_us(lambda: ops.attn_prefill_cached(q, kc, vc, o, B, H, T, d_pos, pos_stride=1))
            row = {"p": p, "T": T, "chunk_attn_us": us,
                   "kv_floor_us": round(2 * B * H * (p + T) * 256 * 2 / HBM_BYTES_PER_S * 1e6, 2)}
            if T == 1:
                od = torch.empty(B, H * 256, dtype=torch.bfloat16, device=dev)
                dp1 = d_pos.clone()
                row["attn_decode_us"] = _launch_us(lambda: ops.attn_decode(q, kc, vc, od, B, H, dp1, pos_stride=1))
            kern.append(row)
    print(json.dumps({"config": args.config, "layers": model.lm.config.num_layers, "batch": B, "gen": gen,
                      "turn1_rows": P + TXT, "question_rows": Q, "legs": legs, "best_ms": best,
                      "continued_over_fresh": round(best["turn2_continued_ms"] / best["turn2_fresh_ms"], 4),
                      "expand_over_full_prompts": round(best["shared_prefix_expand_ms"] / best["shared_prefix_full_prompts_ms"], 4),
                      "chunk_attention": kern}))


def _launch_us(fn, reps=50):
    import torch
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1e3 / reps, 2)


if __name__ == "__main__":
    main()
