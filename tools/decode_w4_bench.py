"""Decode with bf16, W8A16 (e4m3) and W4A16 (MXFP4) weights in ONE process at the bench shape: MAGMA_v1, 28 blocks, B = 8,
32 new tokens.  Per mode: generate() tokens/s (prefill included, as bench.py counts them), ms per captured token step, and
GB/s over the weight bytes that step streams (counted from the operands the planned step reads: codes + scales).

  python tools/decode_w4_bench.py                  # the three modes, token-step timings interleaved
  python tools/decode_w4_bench.py --modes w4       # one mode (e.g. under rocprofv3 --kernel-trace --stats, a run of its own)
  python tools/decode_w4_bench.py --sweep          # also: every W4 GEMV variant on the model's five GEMV shapes

Step timings are device events around ``--steps`` replays of the captured step (windows of about half a second), best of
``--reps`` windows; every mode has its own cache (its plan is fixed when the cache's decode state is made) and the windows of
the modes alternate.  The sweep replays, inside ONE captured graph, the same GEMV over the 28 layers' operands (no launch finds
its weights in the Infinity Cache, no host enqueue between launches) and reports the graph time per launch: a launch's share of
a captured step, which still includes the gap between dependent graph nodes -- it is NOT a kernel time (those come from
rocprofv3 --kernel-trace --stats, in a run of its own), and for the small operands it is mostly that gap."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magma_amd import Magma, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="bf16,w8,w4")
ap.add_argument("--config", default="MAGMA_v1")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--gen", type=int, default=32)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--steps", type=int, default=250)
ap.add_argument("--layers", type=int, default=0, help="0 = the config's depth (28)")
ap.add_argument("--sweep", action="store_true")
args = ap.parse_args()
modes = [m for m in args.modes.split(",") if m]
assert all(m in ("bf16", "w8", "w4") for m in modes)

if not torch.cuda.is_available():
    sys.exit("decode_w4_bench: no GPU -- this tool measures, it does not fall back")
dev = torch.device("cuda:0")
torch.manual_seed(1234)
kw = {}
if args.layers:
    from magma_amd.language_model import GPTJConfig
    kw["lm_config"] = GPTJConfig(num_layers=args.layers, vocab_size=50258)
model = Magma(args.config, device=dev, **kw)
model.eval()
eng = model.lm.engine
B = args.batch
g = torch.Generator(device=dev).manual_seed(1)
images = torch.randn(B, 3, 224, 224, device=dev, generator=g).to(torch.bfloat16)
prompt = torch.randint(0, 50256, (B, 8), device=dev, generator=g)


def set_mode(m):
    eng.decode_w8, eng.decode_w4 = m == "w8", m == "w4"
    eng._cache_pool.clear()          # a pooled cache keeps the plan it was made with


def pack_bytes(p):
    n = p.ft.numel() * p.ft.element_size()
    if isinstance(p, ops.PackedLinearW8):
        n += p.scale.numel() * 4
    if isinstance(p, ops.PackedLinearW4):
        n += p.scales.numel()
    return n


def step_bytes(st):
    """Weight bytes one planned token step streams (every GEMV operand once; activations and the KV cache not counted)."""
    total = 0
    for ly, kind in zip(eng.layers, st.kinds):
        src = ly.w8 if st.w8 else ly.w4 if st.w4 else ly
        if kind == "fold2":
            packs = [ly.dec_in, ly.fc_out, ly.mlp_adapter[0], ly.out_up]
        elif kind == "grouped":
            packs = [src.dec_in, src.fc_out, src.out, src.mlp_adapter[0], src.mlp_adapter[1]]
        elif kind == "v2":
            packs = [src.dec_in, src.fc_out, src.out, src.mlp_adapter[0], src.attn_adapter[0], src.up_cat]
        else:
            raise SystemExit(f"decode_w4_bench: block kind {kind!r} is not counted here")
        total += sum(pack_bytes(p) for p in packs)
    head = eng.head_w8 if st.w8 else eng.head_w4 if st.w4 else eng.head_dec
    return total + pack_bytes(head)


e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
res = {}
with torch.no_grad():
    emb = model.embed([images, prompt])
    S0 = int(emb.shape[1])
    caches = {}
    for m in modes:                                   # one cache per mode: prefill, eager step, capture, replay
        set_mode(m)
        out = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=args.steps + 8)
        cache = out.past_key_values
        tok = out.logits[:, -1].argmax(-1, keepdim=True)
        for _ in range(3):
            eng.decode(tok, cache)
        st = cache.decode_state
        caches[m] = (cache, tok)
        res[m] = {"kinds": sorted(set(st.kinds)), "step_bytes": step_bytes(st), "step_ms_all": []}
    for rep in range(args.reps):                      # interleaved windows
        for m in modes:
            cache, tok = caches[m]
            cache.pos = S0
            cache.d_pos.fill_(S0)                     # same context length in every window
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                eng.decode(tok, cache)
            e1.record()
            torch.cuda.synchronize()
            res[m]["step_ms_all"].append(e0.elapsed_time(e1) / args.steps)
    caches.clear()
    for m in modes:                                   # the public call, prefill included
        set_mode(m)
        gen = lambda: model.generate(emb, max_steps=args.gen, temperature=0.0, decode=False, stop_on_eos=False)  # noqa: E731
        for _ in range(2):
            toks = gen()
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            toks = gen()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        r = res[m]
        r["step_ms"] = min(r["step_ms_all"])
        r["step_tokens_per_s"] = B / (r["step_ms"] * 1e-3)
        r["weight_GB_per_step"] = r["step_bytes"] / 1e9
        r["weight_GB_per_s"] = r["step_bytes"] / (r["step_ms"] * 1e-3) / 1e9
        r["generate_ms"] = min(times) * 1e3
        r["generate_tokens_per_s"] = B * args.gen / min(times)
        r["tokens_checksum"] = int(toks[:, S0:].sum())
        print(json.dumps({"mode": m, **r}), flush=True)
    set_mode("bf16")

    if args.sweep and "w4" in modes:
        # every W4 variant on each GEMV shape of the model: the 28 layers' operands in turn inside one captured graph
        eng._ensure_decode_packs_w4()
        sweep_replays = 200
        shapes = {"dec_in": lambda q: q.dec_in, "fc_out": lambda q: q.fc_out, "out": lambda q: q.out,
                  "ad_dn": lambda q: q.mlp_adapter[0], "ad_up": lambda q: q.mlp_adapter[1]}
        for name, pick in shapes.items():
            packs = [pick(ly.w4) for ly in eng.layers if pick(ly.w4) is not None]
            if not packs:
                continue
            p0 = packs[0]
            x = torch.randn(B, p0.Kp, device=dev).to(torch.bfloat16)
            y = torch.empty(B, ops.ceil_to(p0.N, 8), dtype=torch.bfloat16, device=dev)[:, : p0.N]
            per_wave = p0.Kp // 128
            for kc, nt in [(0, 0), (4, 1), (8, 1), (16, 1), (32, 1), (4, 2), (8, 2), (16, 2), (32, 2), (4, 4), (8, 4), (16, 4)]:
                if kc and per_wave % kc:
                    continue
                v = nt | 4 << 4 | kc << 8 if kc else 0
                for p in packs[:2]:                       # code objects loaded before the capture
                    ops.gemm_skinny(x, p, out=y, use_bias=False, variant=v)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for p in packs:
                        ops.gemm_skinny(x, p, out=y, use_bias=False, variant=v)
                graph.replay()
                best = 1e9
                for _ in range(3):
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(sweep_replays):
                        graph.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    best = min(best, e0.elapsed_time(e1) / (sweep_replays * len(packs)))
                print(json.dumps({"sweep": name, "N": p0.N, "K": p0.K, "kc": kc, "nt": nt, "launches_per_graph": len(packs),
                                  "us_per_launch_in_graph": best * 1e3,
                                  "weight_GB_per_s_of_that": pack_bytes(p0) / (best * 1e-3) / 1e9}), flush=True)
