"""Lossless decode packing (MAGMA_DECODE_PACK) against the bf16 token step in ONE process at the bench shape: MAGMA_v1, 28 blocks,
B = 8.  Prints JSON lines:

  {"mode": ...}    ms per captured token step, packed and bf16, windows interleaved (each mode has its own cache: the captured
                   graphs hold the descriptors they were captured with), the share of weight bytes streamed packed, and whether
                   the two modes' step logits are bit-equal
  {"sweep": ...}   with --sweep: every GEMV shape of the step, the 28 layers' operands in turn inside one captured graph (no launch
                   finds its weights in the Infinity Cache), bf16 and every packed (waves, burst, n-tiles) with the bf16 launch's
                   waves: graph time per launch (a launch's share of a captured step, not a kernel time)

  python tools/decode_pack_bench.py [--sweep] [--layers N]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magma_amd import Magma, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="MAGMA_v1")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--layers", type=int, default=0, help="0 = the config's depth (28)")
ap.add_argument("--sweep", action="store_true")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("decode_pack_bench: no GPU -- this tool measures, it does not fall back")
dev = torch.device("cuda:0")
torch.manual_seed(1234)
kw = {}
if args.layers:
    from magma_amd.language_model import GPTJConfig
    kw["lm_config"] = GPTJConfig(num_layers=args.layers, vocab_size=50258)
model = Magma(args.config, device=dev, **kw)
model.eval()
eng = model.lm.engine
eng.decode_pack = True
B = args.batch
g = torch.Generator(device=dev).manual_seed(1)
images = torch.randn(B, 3, 224, 224, device=dev, generator=g).to(torch.bfloat16)
prompt = torch.randint(0, 50256, (B, 8), device=dev, generator=g)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

with torch.no_grad():
    emb = model.embed([images, prompt])
    S0 = int(emb.shape[1])
    caches, res = {}, {}
    for m in ("packed", "bf16"):
        ops.DECODE_PACK = m == "packed"
        eng._cache_pool.clear()
        out = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=args.steps + 8)
        cache = out.past_key_values
        tok = out.logits[:, -1].argmax(-1, keepdim=True)
        for _ in range(3):
            lg = eng.decode(tok, cache)[0].clone()
        caches[m] = (cache, tok)
        res[m] = {"kinds": sorted(set(cache.decode_state.kinds)), "logits": lg, "step_ms_all": []}
    ops.DECODE_PACK = True
    for rep in range(args.reps):
        for m, (cache, tok) in caches.items():
            cache.pos = S0
            cache.d_pos.fill_(S0)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                eng.decode(tok, cache)
            e1.record()
            torch.cuda.synchronize()
            res[m]["step_ms_all"].append(e0.elapsed_time(e1) / args.steps)
    same = bool(torch.equal(res["packed"]["logits"], res["bf16"]["logits"]))
    for m, r in res.items():
        r.pop("logits")
        print(json.dumps({"mode": m, "step_ms": min(r["step_ms_all"]), **r, "logits_bit_equal": same,
                          "packed_share_of_weight_bytes": eng.decode_pack_share() if m == "packed" else 0.0}), flush=True)
    caches.clear()

    if args.sweep:
        replays = 100
        ly0 = eng.layers[0]
        r = ly0.mlp_adapter[0].N
        shapes = {"dec_in": lambda ly: ly.dec_in, "fc_out": lambda ly: ly.fc_out, "ad_dn": lambda ly: ly.mlp_adapter[0],
                  "out_up": lambda ly: ly.out_up}
        for name, pick in shapes.items():
            packs = [pick(ly) for ly in eng.layers]
            p0 = packs[0]
            x = torch.randn(B, p0.Kp, device=dev).to(torch.bfloat16)
            y = torch.empty(B, ops.ceil_to(p0.N, 8), dtype=torch.bfloat16, device=dev)[:, : p0.N]
            ks = p0.Kp // 32
            waves = 4 if ks % 64 == 0 and ks >= 512 else 8            # the bf16 launch's choice (mg_gemm_skinny_bf16)
            per_wave = ks // waves
            cases = [("bf16", 0)] + [("packed", 0)] + [("packed", nt | waves << 4 | kc << 8) for kc, nt in
                                                     ((4, 1), (4, 2), (8, 1), (8, 2), (16, 1), (16, 2), (20, 1), (32, 1))
                                                     if per_wave % kc == 0 and (waves, kc, nt) in
                                                     {(8, 4, 1), (8, 4, 2), (8, 8, 1), (8, 8, 2), (8, 16, 1), (8, 20, 1),
                                                      (4, 4, 1), (4, 8, 1), (4, 16, 1), (4, 16, 2), (4, 32, 1)}]
            for mode, v in cases:
                ops.DECODE_PACK = mode == "packed"
                for p in packs[:2]:
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
                    for _ in range(replays):
                        graph.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    best = min(best, e0.elapsed_time(e1) / (replays * len(packs)))
                print(json.dumps({"sweep": name, "N": p0.N, "K": p0.K, "mode": mode, "waves": waves, "kc": (v >> 8) & 255,
                                  "nt": v & 15, "us_per_launch_in_graph": best * 1e3,
                                  "bf16_GB_per_s": p0.ft.numel() * 2 / (best * 1e-3) / 1e9}), flush=True)
        ops.DECODE_PACK = True
