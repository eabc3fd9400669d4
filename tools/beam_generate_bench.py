"""Beam-search token step against the greedy token step at the same row count (DESIGN.md "Beam search"): MAGMA_v1, prefill 57,
B = 4 x k = 4 (16 rows: the captured weight-streaming step) and B = 8 x k = 4 (32 rows: the eager tile-GEMM step).

    python tools/beam_generate_bench.py [--layers 28] [--gen 32] [--steps 3] [--warmup 1] [--out profiles/beam_step.jsonl]

Per shape: ms per token step of greedy and of beam decoding (generate() minus its prefill, over `gen` steps, the eos stop
switched off for greedy and never reached for beam -- eos is a token the random model does not favour), the GPU time of the
beam step's three selection / bookkeeping / reorder launches and their share of the step, and the bytes the KV reorder
copied per step.  One JSON line per shape (appended to --out as well)."""
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
    ap.add_argument("--shapes", default="4x4,8x4", help="comma-separated BxK")
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

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    def prefill_only(emb):
        return model.lm(inputs_embeds=emb, use_cache=True, cache_hint=gen, reuse_cache=True, eos_token=model.eos_token)

    lines = []
    for shape in args.shapes.split(","):
        B, k = (int(v) for v in shape.split("x"))
        R = B * k
        g = torch.Generator(device=dev).manual_seed(7)
        emb = torch.randn(B, S, d, device=dev, generator=g).to(torch.bfloat16)
        emb_r = emb.repeat_interleave(k, dim=0)
        # greedy at R rows (no early stop) and beam at B x k, whole generate(); the prefill of R rows is common to both
        t_greedy = timed(lambda: model.generate(emb_r, max_steps=gen, temperature=0.0, decode=False, stop_on_eos=False))
        t_beam = timed(lambda: model.generate(emb, max_steps=gen, num_beams=k, decode=False, early_stopping="never",
                                              length_penalty=0.0))
        t_pre = timed(lambda: prefill_only(emb_r))
        step_greedy = (t_greedy - t_pre) / (gen - 1)
        step_beam = (t_beam - t_pre) / (gen - 1)

        # the three launches alone, on the cache the last beam call left (GPU time by events; state restored between runs)
        cache = eng._cache_pool[next(c for c in eng._cache_pool if c[0] == R)]
        bm, st = cache.beam, cache.decode_state
        mode = eng.beam_mode((k, 0.0, "never", gen))
        logits = st.logits[:, : eng.V]
        saved = {n: t.clone() for n, t in bm.bufs.items() if n not in ("hist",)}
        state0 = cache.sample_state.clone()

        def restore():
            for n, t in saved.items():
                bm.bufs[n].copy_(t)
            cache.sample_state.copy_(state0)
            cache.sample_state[1] = -1

        def ev_time(fn, n=10):
            ts = []
            for _ in range(n):
                restore()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
            return sorted(ts)[len(ts) // 2]

        t_sel = ev_time(lambda: ops.beam_topk(logits, bm.run, bm.cand_score, bm.cand_tok))
        t_fin = ev_time(lambda: ops.beam_finish(bm.cand_score, bm.cand_tok, bm.B, k, eng.V, cache.eos, 0.0, "never", gen,
                                                cache.sample_state, bm.bufs))
        t_reo = ev_time(lambda: ops.kv_reorder(cache.k, cache.v, bm.kstage, bm.vstage, bm.parent, cache.d_pos))
        restore()

        # bytes the reorder wrote per step: one eager beam run that reads the parent map after every step
        per_pos = eng.L * eng.H * 256 * 2 * 2                     # K and V, bf16, one position of one row in every layer
        moved = []
        o = model.lm(inputs_embeds=emb_r, use_cache=True, cache_hint=gen, reuse_cache=True, eos_token=model.eos_token,
                     beam=(k, 0.0, "never", gen))
        past = o.past_key_values
        for i in range(gen):
            par = past.beam.parent.cpu().tolist()
            n_pos = int(past.d_pos[0]) if not past.ragged else int(past.d_pos.max())
            rows = sum(1 for b, p in enumerate(par) if p != b)
            staged = sum(1 for b, p in enumerate(par) if p != b and any(c != b and par[c] == b for c in range(R)))
            moved.append((rows + staged) * n_pos * per_pos)
            if i + 1 == gen:
                break
            o = model.lm(input_ids=None, use_cache=True, past_key_values=past, feed_back=True, beam=(k, 0.0, "never", gen))
        line = {"config": args.config, "layers": model.lm.config.num_layers, "B": B, "num_beams": k, "rows": R, "gen": gen,
                "prefill_ms": round(t_pre * 1e3, 3), "greedy_step_ms": round(step_greedy * 1e3, 3),
                "beam_step_ms": round(step_beam * 1e3, 3), "beam_over_greedy": round(step_beam / step_greedy, 4),
                "select_ms": round(t_sel, 4), "bookkeeping_ms": round(t_fin, 4), "reorder_ms": round(t_reo, 4),
                "launch_share": {"select": round(t_sel / (step_beam * 1e3), 4), "bookkeeping": round(t_fin / (step_beam * 1e3), 4),
                                 "reorder": round(t_reo / (step_beam * 1e3), 4)},
                "reorder_bytes_written_per_step": {"mean": int(sum(moved) / len(moved)), "max": int(max(moved))},
                "step_graph": R <= 16}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
