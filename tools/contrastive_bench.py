"""Contrastive search (DESIGN.md "Contrastive search"): what the captured token step costs beside the greedy step over the same
number of rows, and the similarity kernel alone.  MAGMA_v1, random weights, 28 blocks, full width, prompt of 57 rows.

    python tools/contrastive_bench.py [--layers 28] [--cases 2x4,4x4,2x8,1x16] [--steps 200] [--reps 3] [--out profiles/contrastive_bench.jsonl]

Per (B, k): two caches of R = B * k rows in ONE process, one armed for contrastive search (top_k = k, penalty_alpha = 0.6), one for
greedy decoding; after an eager step, the capture and a replay of each, windows of ``--steps`` replays alternate between the two
(device events around a window, positions and context lengths reset before each, best of ``--reps``).  The difference of the two
step times is what the candidates' selection costs; the greedy step's weight bytes over its time is the bandwidth the decode
GEMVs reach on this machine (counted as tools/decode_w4_bench.py counts them).

The similarity kernel alone, B = 2, k = 4, d = 4096, a store of 2048 positions, context lengths 57, 512 and 2047: ONE captured
graph of ``--sim-launches`` launches that walk over enough context stores to exceed the 256 MB Infinity Cache (no launch finds its
context there), replayed; the time per launch in the graph still includes the gap between dependent graph nodes -- it is not a
kernel time -- and is set against the time to stream the launch's own context bytes at the bandwidth measured above.

One JSON line per case is printed and appended to --out.  No GPU: the tool fails, it does not fall back."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="MAGMA_v1")
    ap.add_argument("--layers", type=int, default=None, help="GPT-J blocks (default: the config's 28)")
    ap.add_argument("--prompt", type=int, default=57)
    ap.add_argument("--cases", default="2x4,4x4,2x8,1x16")
    ap.add_argument("--alpha", type=float, default=0.6)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sim-launches", type=int, default=96)
    ap.add_argument("--sim-replays", type=int, default=40)
    ap.add_argument("--out", default=os.path.join("profiles", "contrastive_bench.jsonl"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("contrastive_bench: no GPU -- this tool measures, it does not fall back")
    from magma_amd import Magma, ops
    from magma_amd.engine import LMEngine
    from magma_amd.language_model import GPTJConfig
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    lm_cfg = GPTJConfig(num_layers=args.layers, vocab_size=50258) if args.layers else None
    model = Magma(args.config, device=dev, lm_config=lm_cfg)
    model.eval()
    eng = model.lm.engine
    d, S0 = eng.d, args.prompt
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    def step_bytes(st):
        """Weight bytes one planned token step streams (every GEMV operand once; activations and the KV cache not counted)."""
        nbytes = lambda p: p.ft.numel() * p.ft.element_size()  # noqa: E731
        total = 0
        for ly, kind in zip(eng.layers, st.kinds):
            if kind != "fold2":
                raise SystemExit(f"contrastive_bench: block kind {kind!r} is not counted here")
            total += sum(nbytes(p) for p in (ly.dec_in, ly.fc_out, ly.mlp_adapter[0], ly.out_up))
        return total + nbytes(eng.head_dec)

    gbps = None
    with torch.no_grad():
        for case in args.cases.split(","):
            B, k = (int(v) for v in case.split("x"))
            R = B * k
            g = torch.Generator(device=dev).manual_seed(7)
            emb = (torch.randn(B, S0, d, device=dev, generator=g) * 0.5).to(torch.bfloat16).repeat_interleave(k, dim=0)
            plans = {"contrastive": LMEngine.selection_plan(contrast=(k, args.alpha), vocab=eng.V),
                     "greedy": LMEngine.selection_plan(vocab=eng.V)}
            caches = {}
            for name, plan in plans.items():          # a cache of its own per leg: prefill, eager step, capture, replay
                o = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=args.steps + 8, eos_token=model.eos_token, plan=plan)
                caches[name] = o.past_key_values
                for _ in range(3):
                    eng.decode(None, caches[name], plan=plan)
            ms = {name: [] for name in plans}
            for _ in range(args.reps):                # interleaved windows, the same context lengths in every one
                for name, plan in plans.items():
                    cache = caches[name]
                    cache.pos = S0
                    cache.d_pos.fill_(S0)
                    cache.sample_state.copy_(torch.tensor([0, -1], dtype=torch.int32))
                    if name == "contrastive":
                        cache.contrast.ctx_len.fill_(S0)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(args.steps):
                        eng.decode(None, cache, plan=plan)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(round(e0.elapsed_time(e1) / args.steps, 4))
            st = caches["greedy"].decode_state
            best = {name: min(v) for name, v in ms.items()}
            wb = step_bytes(st)
            rate = wb / (best["greedy"] * 1e-3) / 1e9
            if (B, k) == (2, 4) or gbps is None:
                gbps = rate
            emit({"case": "step", "config": args.config, "layers": eng.L, "prompt_rows": S0, "B": B, "k": k, "rows": R,
                  "alpha": args.alpha, "steps_per_window": args.steps, "ms_per_token_all": ms, "ms_per_token": best,
                  "contrastive_minus_greedy_ms": round(best["contrastive"] - best["greedy"], 4),
                  "contrastive_over_greedy": round(best["contrastive"] / best["greedy"], 4),
                  "weight_GB_per_step": round(wb / 1e9, 3), "greedy_weight_GB_per_s": round(rate, 1)})
            caches.clear()
            torch.cuda.empty_cache()

        # ---- the similarity kernel alone
        B, k, Tmax = 2, 4, 2048
        n_chunk = ops.contrastive_chunks(Tmax)
        hidden = torch.randn(B * k, d, device=dev).to(torch.bfloat16)
        part = torch.zeros(B, n_chunk, k, device=dev)
        n_store = max(2, (320 << 20) // (B * Tmax * d * 2) + 1)          # together larger than the Infinity Cache
        stores = torch.randn(n_store, B, Tmax, d, device=dev, dtype=torch.bfloat16)
        for T in (57, 512, 2047):
            ctx_len = torch.full((B,), T, dtype=torch.int32, device=dev)
            for i in range(2):                                         # code object loaded before the capture
                ops.contrastive_sim(hidden, stores[i], ctx_len, k, part, T)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for i in range(args.sim_launches):
                    ops.contrastive_sim(hidden, stores[i % n_store], ctx_len, k, part, T)
            graph.replay()
            best = 1e9
            for _ in range(args.reps):
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.sim_replays):
                    graph.replay()
                e1.record()
                torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1) / (args.sim_replays * args.sim_launches))
            ctx_bytes = B * T * d * 2
            stream_us = ctx_bytes / (gbps * 1e9) * 1e6
            emit({"case": "sim", "B": B, "k": k, "d": d, "T": T, "Tmax": Tmax, "chunks_per_sample": n_chunk,
                  "workgroups_with_work": B * ((T + ops.CONTRASTIVE_CHUNK - 1) // ops.CONTRASTIVE_CHUNK),
                  "context_stores_walked": n_store, "launches_per_graph": args.sim_launches,
                  "us_per_launch_in_graph": round(best * 1e3, 3), "context_MB": round(ctx_bytes / 1e6, 3),
                  "stream_us_at_decode_bandwidth": round(stream_us, 3), "decode_weight_GB_per_s": round(gbps, 1),
                  "launch_over_stream": round(best * 1e3 / stream_us, 2)})


if __name__ == "__main__":
    main()
