"""Token step with and without the logits processors (DESIGN.md "Logits processors"): MAGMA_v1, B = 8, prefill 57, 32 tokens.

    python tools/logits_process_bench.py [--layers 28] [--gen 32] [--steps 3] [--warmup 1] [--out profiles/logits_process_bench.jsonl]

Two shapes: the greedy step at 8 rows and the beam step at 4 x 4 = 16 rows, each timed plain and with all four rules
(repetition_penalty 1.3, no_repeat_ngram_size 3, min_new_tokens 8, 16 suppress ids), the two interleaved round by round on the same
box: ms per token step (generate() minus its prefill, over `gen` steps; the eos stop switched off for greedy, never reached for
beam) and the GPU time of the processor launch alone by events (raw form on the greedy rows, beam form on the beam rows).  One
JSON line per shape (appended to --out as well)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="MAGMA_v1")
    ap.add_argument("--layers", type=int, default=None, help="GPT-J blocks (default: the config's 28)")
    ap.add_argument("--gen", type=int, default=32)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from magma_amd import Magma, ops
    from magma_amd.language_model import GPTJConfig
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    lm_cfg = GPTJConfig(num_layers=args.layers, vocab_size=50258) if args.layers else None
    model = Magma(args.config, device=dev, lm_config=lm_cfg)
    model.eval()
    eng = model.lm.engine
    S, gen = 57, args.gen
    d = model.lm.config.hidden_size
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=8, suppress_tokens=list(range(100, 116)))

    def interleaved(fns):
        """Seconds per call of every fn: warm-up, then `steps` rounds that run each of them once."""
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        total = [0.0] * len(fns)
        for _ in range(args.steps):
            for i, fn in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                total[i] += time.perf_counter() - t0
        return [t / args.steps for t in total]

    def ev_time(fn, n=20):
        ts = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return sorted(ts)[len(ts) // 2]

    lines = []
    for name, B, k in (("greedy", 8, 1), ("beam", 4, 4)):
        R = B * k
        g = torch.Generator(device=dev).manual_seed(7)
        emb = torch.randn(B, S, d, device=dev, generator=g).to(torch.bfloat16)
        emb_r = emb.repeat_interleave(k, dim=0)
        if k == 1:
            kw = dict(temperature=0.0, stop_on_eos=False)
        else:
            kw = dict(num_beams=k, early_stopping="never", length_penalty=0.0)
        t_plain, t_proc, t_pre = interleaved([
            lambda: model.generate(emb, max_steps=gen, decode=False, **kw),
            lambda: model.generate(emb, max_steps=gen, decode=False, **kw, **rules),
            lambda: model.lm(inputs_embeds=emb_r, use_cache=True, cache_hint=gen, reuse_cache=True, eos_token=model.eos_token)])
        step_plain, step_proc = (t_plain - t_pre) / (gen - 1), (t_proc - t_pre) / (gen - 1)
        # the launch alone at the last step's history (re-processing processed rows costs the same: the work does not depend on values)
        cache = eng._cache_pool[next(c for c in eng._cache_pool if c[0] == R)]
        logits = cache.decode_state.logits[:, : eng.V]
        state = torch.tensor([gen - 1, -1], dtype=torch.int32, device=dev)
        sup = torch.arange(100, 116, dtype=torch.int32, device=dev)
        t_launch = ev_time(lambda: ops.logits_process(logits, state, cache.history, repetition_penalty=1.3, no_repeat_ngram_size=3,
                                                      min_new_tokens=8, eos=model.eos_token, suppress=sup, normalize=k > 1))
        line = {"config": args.config, "layers": model.lm.config.num_layers, "mode": name, "B": B, "num_beams": k, "rows": R,
                "gen": gen, "prefill_ms": round(t_pre * 1e3, 3), "plain_step_ms": round(step_plain * 1e3, 4),
                "processed_step_ms": round(step_proc * 1e3, 4), "added_us_per_step": round((step_proc - step_plain) * 1e6, 2),
                "processed_over_plain": round(step_proc / step_plain, 4), "process_launch_us": round(t_launch * 1e3, 2),
                "rules": {k_: (v if not isinstance(v, list) else len(v)) for k_, v in rules.items()}}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
