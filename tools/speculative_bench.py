"""Speculative greedy decoding (DESIGN.md "Speculative decoding"): what the speculative token step costs beside the plain greedy
steps, the chunk attention launch alone, and generate() end to end.  MAGMA_v1, random weights, 28 blocks, full width, prompt of 57.

    python tools/speculative_bench.py [--layers 28] [--cases 1x8,2x4,2x8,4x4] [--steps 200] [--reps 5] [--out profiles/speculative_bench.jsonl]

One process.  Per (B, T) four caches, each after an eager step, the capture and a replay: (a) the plain per-row greedy step over B
rows, (b) the same over B * T rows -- it streams the same weights as (c) and runs T times the attention workgroups --, (c) the
speculative step over B sequences of T rows, (d) the same with MAGMA_SPEC_COLAUNCH=0: the chunk attention and the GEMV as two launches
instead of the co-launch, whose GEMV workgroups carry the chunk body's LDS block and registers.  Windows of ``--steps`` replays alternate between the legs (device events around a
window, positions and loop state reset before each); reported are every window, the median of ``--reps`` and (b)'s own spread.
(c) / (a) is the break-even: speculation pays when the mean tokens per step and row exceed it.

The chunk launch alone, B = 2, T = 8, contexts of 57, 512 and 2047: ONE captured graph of ``--attn-launches`` launches over as many
caches as exceed the 256 MB Infinity Cache, replayed, against the same graph with T single-query launches in place of each chunk
launch.  The time per launch in a graph includes the gap between dependent nodes; it is not a kernel time.

End to end: tokens per second of a 64-token generate() at B = 1 and 2 -- the plain per-row greedy call, the speculative call with
``lookup_ids`` = the plain greedy output (every draft accepted: the ceiling) and with none --, the median of ``--reps`` wall-clock
times after a warm-up call each, with the acceptance counts of ``Speculation``.  The weights are synthetic: acceptance on real
prompts is NOT what the no-lookup number shows.

Sampled rows (case "step_sampled"): per (B, T), in the same way, the plain per-row greedy step over B * T rows (b), the plain
per-row SAMPLED step over B * T rows (e: mg_sample_rows_f32 where mg_argmax_f32 stood), the greedy speculative step (c) and the
sampled speculative step (f: mg_sample_chunk_f32 where mg_argmax_f32 stood), every record temperature 0.7, top_p 0.9.  The
expectation to check: f - c exceeds e - b by no more than the larger leg's own window spread.  Case "e2e_sampled": the 64-token call
with those settings and one seed per row -- the plain per-row sampled call, the speculative call with ``lookup_ids`` = that
call's own output (the mode is seed-exact, so this is a true ceiling) and with none.

One JSON line per case is printed and appended to --out.  No GPU: the tool fails, it does not fall back."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="MAGMA_v1")
    ap.add_argument("--layers", type=int, default=None, help="GPT-J blocks (default: the config's 28)")
    ap.add_argument("--prompt", type=int, default=57)
    ap.add_argument("--cases", default="1x8,2x4,2x8,4x4")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--attn-launches", type=int, default=64)
    ap.add_argument("--attn-replays", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--skip", default="", help="comma list of parts to leave out: step, attn, e2e, step_sampled, e2e_sampled")
    ap.add_argument("--out", default=os.path.join("profiles", "speculative_bench.jsonl"))
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))

    import torch
    if not torch.cuda.is_available():
        sys.exit("speculative_bench: no GPU -- this tool measures, it does not fall back")
    from magma_amd import Magma, ops
    from magma_amd.engine import LMEngine
    from magma_amd.language_model import GPTJConfig
    from magma_amd.sampling import generate
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    lm_cfg = GPTJConfig(num_layers=args.layers, vocab_size=50258) if args.layers else None
    model = Magma(args.config, device=dev, lm_config=lm_cfg)
    model.eval()
    eng = model.lm.engine
    d, S0 = eng.d, args.prompt
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    med = lambda v: round(statistics.median(v), 4)  # noqa: E731

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    def prompts(B):
        g = torch.Generator(device=dev).manual_seed(7)
        return (torch.randn(B, S0, d, device=dev, generator=g) * 0.5).to(torch.bfloat16)

    eos = eng.V - 1                       # an id the loop may meet; the steps run the same launches for finished rows
    stop = dict(eos_ids=(eos,), stop_seqs=())
    with torch.no_grad():
        # ---- the step: (a) plain over B rows, (b) plain over B * T rows, (c) speculative
        for case in ([] if "step" in skip else args.cases.split(",")):
            B, T = (int(v) for v in case.split("x"))
            plain = LMEngine.selection_plan(stop=stop, vocab=eng.V)
            spec = LMEngine.selection_plan(stop=stop, speculate=(T, 2), vocab=eng.V)
            legs = {}
            for name, rows, plan in (("a_plain_B", B, plain), ("b_plain_BT", B * T, plain), ("c_speculative", B, spec),
                                     ("d_speculative_two_launches", B, spec)):
                # (d): MAGMA_SPEC_COLAUNCH=0, read when the cache's speculative state is created -- the chunk attention, then the GEMV
                os.environ["MAGMA_SPEC_COLAUNCH"] = "0" if name.startswith("d_") else "1"
                lens = torch.full((rows,), S0, dtype=torch.int64)
                kw = dict(seed=dict(limit=args.steps, lookup=None)) if plan is spec else {}
                o = model.lm(inputs_embeds=prompts(B).repeat_interleave(rows // B, 0), use_cache=True, cache_hint=args.steps + T + 8,
                             eos_token=eos, plan=plan, lengths=lens, **kw)
                legs[name] = (o.past_key_values, plan)
                for _ in range(3):        # eager, capture, replay
                    eng.decode(None, o.past_key_values, plan=plan)

            def reset(cache, plan):
                cache.pos = S0
                cache.d_pos.fill_(S0)
                cache.sample_state.copy_(torch.tensor([0, -1], dtype=torch.int32))
                cache.finish.copy_(torch.tensor([[-1, 0]] * cache.B, dtype=torch.int32))
                if plan is spec:
                    st = cache.spec[T]
                    for t in (st.n_draft, st.count, st.stats, st.ids):
                        t.zero_()
            ms = {name: [] for name in legs}
            for _ in range(args.reps):
                for name, (cache, plan) in legs.items():
                    reset(cache, plan)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(args.steps):
                        eng.decode(None, cache, plan=plan)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(round(e0.elapsed_time(e1) / args.steps, 4))
            m = {name: med(v) for name, v in ms.items()}
            stats = legs["c_speculative"][0].spec[T].stats.cpu().tolist()
            emit({"case": "step", "config": args.config, "layers": eng.L, "prompt_rows": S0, "B": B, "T": T, "rows": B * T,
                  "steps_per_window": args.steps, "windows": args.reps, "ms_per_step_all": ms, "ms_per_step_median": m,
                  "b_spread_ms": round(max(ms["b_plain_BT"]) - min(ms["b_plain_BT"]), 4),
                  "c_minus_b_ms": round(m["c_speculative"] - m["b_plain_BT"], 4),
                  "d_minus_c_ms": round(m["d_speculative_two_launches"] - m["c_speculative"], 4),
                  "break_even_tokens_per_step_c_over_a": round(m["c_speculative"] / m["a_plain_B"], 4),
                  "last_window_stats_steps_drafted_accepted": stats})
            legs.clear()
            os.environ.pop("MAGMA_SPEC_COLAUNCH", None)
            torch.cuda.empty_cache()

        # ---- the sampled step: (b) plain greedy and (e) plain per-row sampled over B * T rows, (c) greedy and (f) sampled speculative
        for case in ([] if "step_sampled" in skip else args.cases.split(",")):
            B, T = (int(v) for v in case.split("x"))
            table = lambda n: ops.sample_rows_table([0.7] * n, [0] * n, [0.9] * n, [0.0] * n, list(range(11, 11 + n)))  # noqa: E731
            plans = {"b_plain_BT": LMEngine.selection_plan(stop=stop, vocab=eng.V),
                     "e_plain_rows_BT": LMEngine.selection_plan(stop=stop, sampling=("rows", False), vocab=eng.V),
                     "c_speculative": LMEngine.selection_plan(stop=stop, speculate=(T, 2), vocab=eng.V),
                     "f_speculative_rows": LMEngine.selection_plan(stop=stop, speculate=(T, 2), sampling=("rows", False), vocab=eng.V)}
            seeds = {"b_plain_BT": {}, "e_plain_rows_BT": dict(seed=table(B * T)), "c_speculative": dict(seed=dict(limit=args.steps, lookup=None)),
                     "f_speculative_rows": dict(seed=dict(limit=args.steps, lookup=None, rows=table(B)))}
            legs = {}
            for name, plan in plans.items():
                rows = B if plan.is_speculate else B * T
                o = model.lm(inputs_embeds=prompts(B).repeat_interleave(rows // B, 0), use_cache=True, cache_hint=args.steps + T + 8,
                             eos_token=eos, plan=plan, lengths=torch.full((rows,), S0, dtype=torch.int64), **seeds[name])
                legs[name] = (o.past_key_values, plan)
                for _ in range(3):        # eager, capture, replay
                    eng.decode(None, o.past_key_values, plan=plan)
            assert len({id(c) for c, _ in legs.values()}) == 4

            def reset_rows(cache, plan):
                cache.pos = S0
                cache.d_pos.fill_(S0)
                cache.sample_state.copy_(torch.tensor([0, -1], dtype=torch.int32))
                cache.finish.copy_(torch.tensor([[-1, 0]] * cache.B, dtype=torch.int32))
                if plan.is_speculate:
                    st = cache.spec[T]
                    for t in (st.n_draft, st.count, st.stats, st.ids):
                        t.zero_()
            ms = {name: [] for name in legs}
            for _ in range(args.reps):
                for name, (cache, plan) in legs.items():
                    reset_rows(cache, plan)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(args.steps):
                        eng.decode(None, cache, plan=plan)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(round(e0.elapsed_time(e1) / args.steps, 4))
            m = {name: med(v) for name, v in ms.items()}
            spread = {name: round(max(v) - min(v), 4) for name, v in ms.items()}
            emit({"case": "step_sampled", "config": args.config, "layers": eng.L, "prompt_rows": S0, "B": B, "T": T, "rows": B * T,
                  "steps_per_window": args.steps, "windows": args.reps, "ms_per_step_all": ms, "ms_per_step_median": m,
                  "spread_ms": spread, "e_minus_b_ms": round(m["e_plain_rows_BT"] - m["b_plain_BT"], 4),
                  "f_minus_c_ms": round(m["f_speculative_rows"] - m["c_speculative"], 4),
                  "last_window_stats_steps_drafted_accepted": legs["f_speculative_rows"][0].spec[T].stats.cpu().tolist()})
            legs.clear()
            torch.cuda.empty_cache()

        # ---- the chunk launch alone against T single-query launches
        if "attn" not in skip:
            B, T, H, Smax = 2, 8, eng.H, 2112
            qkv = (torch.randn(B * T, 3 * d, device=dev) * 0.5).to(torch.bfloat16)
            out = torch.empty(B * T, d, dtype=torch.bfloat16, device=dev)
            n_cache = max(2, (320 << 20) // (2 * B * H * Smax * 256 * 2) + 1)          # together larger than the Infinity Cache
            ks = (torch.randn(n_cache, B, H, Smax, 256, device=dev) * 0.5).to(torch.bfloat16)
            vs = torch.randn(n_cache, B, H, Smax, 256, device=dev).to(torch.bfloat16)
            q1 = [qkv[t::T].contiguous() for t in range(T)]
            o1 = torch.empty(B, d, dtype=torch.bfloat16, device=dev)
            for ctx in (57, 512, 2047):
                p0 = ctx + 1 - T          # the last query of the chunk attends over ctx keys
                pos = torch.full((B,), p0, dtype=torch.int32, device=dev)
                pos_t = [pos + t for t in range(T)]

                def chunk(i):
                    ops.attn_decode_chunk(qkv, ks[i], vs[i], out, B, T, H, pos, eng.rot, eng.sin_t, eng.cos_t, pos_stride=1)

                def singles(i):
                    for t in range(T):
                        ops.attn_decode_fused(q1[t], ks[i], vs[i], o1, B, H, pos_t[t], eng.rot, eng.sin_t, eng.cos_t, pos_stride=1)
                res = {}
                for name, fn in (("chunk", chunk), ("singles", singles)):
                    fn(0)
                    torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        for i in range(args.attn_launches):
                            fn(i % n_cache)
                    graph.replay()
                    res[name] = graph
                us = {name: [] for name in res}
                for _ in range(args.reps):
                    for name, graph in res.items():
                        torch.cuda.synchronize()
                        e0.record()
                        for _ in range(args.attn_replays):
                            graph.replay()
                        e1.record()
                        torch.cuda.synchronize()
                        us[name].append(round(e0.elapsed_time(e1) * 1e3 / (args.attn_replays * args.attn_launches), 3))
                emit({"case": "attn", "B": B, "T": T, "H": H, "Smax": Smax, "context": ctx, "caches_walked": n_cache,
                      "launches_per_graph": args.attn_launches, "us_per_chunk_launch_all": us["chunk"],
                      "us_per_T_single_launches_all": us["singles"], "us_per_chunk_launch": med(us["chunk"]),
                      "us_per_T_single_launches": med(us["singles"]),
                      "singles_over_chunk": round(med(us["singles"]) / med(us["chunk"]), 3)})
            del ks, vs
            torch.cuda.empty_cache()

        # ---- end to end
        for B in ([] if "e2e" in skip else (1, 2)):
            emb, n = prompts(B), args.tokens
            kw = dict(max_steps=n, temperature=0.0, decode=False, eos_token=[eos], stop_per_row=True, stop_on_eos=False)
            ref = generate(model, emb, **kw)
            answer = [ref[b, S0:].tolist() for b in range(B)]

            def timed(**more):
                generate(model, emb, **kw, **more)                      # warm-up: allocation, capture
                ts, last = [], None
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last = generate(model, emb, **kw, **more)
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                return ts, last
            t_plain, _ = timed()
            line = {"case": "e2e", "B": B, "new_tokens": n, "prompt_rows": S0, "layers": eng.L,
                    "plain_tokens_per_s": round(B * n / statistics.median(t_plain), 1), "plain_s_all": [round(t, 5) for t in t_plain]}
            for T in (4, 8):
                for name, lookup in (("lookup_answer", answer), ("lookup_none", None)):
                    ts, (got, sp) = timed(prompt_lookup_num_tokens=T - 1, lookup_ids=lookup, return_speculation=True)
                    line[f"T{T}_{name}"] = {"tokens_per_s": round(B * n / statistics.median(ts), 1), "s_all": [round(t, 5) for t in ts],
                                            "equals_plain": bool(torch.equal(got, ref)), "steps": sp.steps.tolist(),
                                            "drafted": sp.drafted.tolist(), "accepted": sp.accepted.tolist()}
            emit(line)

        # ---- end to end, sampled rows: the plain per-row sampled call, then its own output as the lookup text (seed-exact: the ceiling)
        for B in ([] if "e2e_sampled" in skip else (1, 2)):
            emb, n = prompts(B), args.tokens
            kw = dict(max_steps=n, temperature=[0.7] * B, top_p=[0.9] * B, seed=list(range(11, 11 + B)), decode=False, eos_token=[eos],
                      stop_per_row=True, stop_on_eos=False)
            ref = generate(model, emb, **kw)
            answer = [ref[b, S0:].tolist() for b in range(B)]

            def timed_rows(**more):
                generate(model, emb, **kw, **more)                      # warm-up: allocation, capture
                ts, last = [], None
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last = generate(model, emb, **kw, **more)
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                return ts, last
            t_plain, _ = timed_rows()
            line = {"case": "e2e_sampled", "B": B, "new_tokens": n, "prompt_rows": S0, "layers": eng.L, "temperature": 0.7, "top_p": 0.9,
                    "plain_tokens_per_s": round(B * n / statistics.median(t_plain), 1), "plain_s_all": [round(t, 5) for t in t_plain]}
            for T in (4, 8):
                for name, lookup in (("lookup_answer", answer), ("lookup_none", None)):
                    ts, (got, sp) = timed_rows(prompt_lookup_num_tokens=T - 1, lookup_ids=lookup, return_speculation=True)
                    line[f"T{T}_{name}"] = {"tokens_per_s": round(B * n / statistics.median(ts), 1), "s_all": [round(t, 5) for t in ts],
                                            "equals_plain": bool(torch.equal(got, ref)), "steps": sp.steps.tolist(),
                                            "drafted": sp.drafted.tolist(), "accepted": sp.accepted.tolist()}
            emit(line)


if __name__ == "__main__":
    main()
