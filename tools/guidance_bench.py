"""What classifier-free guidance costs per token, in ONE process at the bench shape: MAGMA_v1, 28 blocks, full width, image + 8
text tokens (context 57 -> 57 + steps), greedy.  Three captured token steps, their timing windows interleaved:

  guided16   generate(guidance_scale=3, guidance_min_p=0.1) over B = 8 samples: 16 ragged rows, the 8 prompts (57 positions)
             and the 8 text-only negative prompts (8 positions), two launches more than
  plain16    the unguided step over the same 16 ragged rows (what the engine launched for them before guidance existed), and
  plain8     the unguided step over the 8 prompts alone.

  python tools/guidance_bench.py
  python tools/guidance_bench.py --arms plain16,plain8     # on a tree without guidance the guided arm is left out by itself

Step timings are device events around ``--steps`` replays of the captured step, one window per arm per repetition, the arms
alternating; reported are every window, their median and their minimum.  The last line times the guidance launch alone:
``--launches`` launches over 8 pairs of V = 50 258 inside one captured graph, graph time per launch -- a launch's share of a
captured step, which includes the gap between dependent graph nodes; it is not a kernel time (that comes from rocprofv3
--kernel-trace --stats, in a run of its own).  That graph runs at scale 1, where the rule maps a row to its log_softmax: applied
over and over in place the rows stay finite, and the arithmetic per element is the same."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magma_amd import Magma, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--arms", default="guided16,plain16,plain8")
ap.add_argument("--config", default="MAGMA_v1")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=250)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--layers", type=int, default=0, help="0 = the config's depth (28)")
args = ap.parse_args()
has_guidance = hasattr(ops, "logits_guidance")
arms = [a for a in args.arms.split(",") if a and (has_guidance or a != "guided16")]
assert all(a in ("guided16", "plain16", "plain8") for a in arms)

if not torch.cuda.is_available():
    sys.exit("guidance_bench: no GPU -- this tool measures, it does not fall back")
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
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

with torch.no_grad():
    emb = model.embed([images, prompt])
    neg = model.embed([prompt])
    S0, S1 = int(emb.shape[1]), int(neg.shape[1])
    both = torch.zeros(2 * B, S0, emb.shape[2], dtype=emb.dtype, device=dev)
    both[:B], both[B:, :S1] = emb, neg
    lens = {"guided16": [S0] * B + [S1] * B, "plain16": [S0] * B + [S1] * B, "plain8": [S0] * B}
    state = {}
    for a in arms:                                   # one cache per arm: prefill, eager step, capture, replay
        rows = emb if a == "plain8" else both
        gd = dict(guidance=(3.0, 0.1)) if a == "guided16" else {}
        ln = torch.tensor(lens[a], dtype=torch.int64)
        out = model.lm(inputs_embeds=rows, use_cache=True, cache_hint=args.steps + 8, lengths=ln, eos_token=model.eos_token, **gd)
        cache = out.past_key_values
        for _ in range(3):
            eng.decode(None, cache, **gd)
        state[a] = (cache, gd, ln.to(torch.int32).to(dev), [])
    for rep in range(args.reps):                     # interleaved windows
        for a in arms:
            cache, gd, ln, times = state[a]
            cache.pos = S0
            cache.d_pos.copy_(ln)                    # same context lengths in every window
            cache.sample_state.copy_(torch.tensor([0, -1], dtype=torch.int32))
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                eng.decode(None, cache, **gd)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / args.steps)
    for a in arms:
        cache, gd, ln, times = state[a]
        print(json.dumps({"arm": a, "rows": cache.B, "samples": B, "context": [S0, S0 + args.steps], "steps_per_window": args.steps,
                          "step_ms_median": statistics.median(times), "step_ms_min": min(times), "step_ms_all": times,
                          "graphs": len(cache.decode_state.graphs)}), flush=True)
    if has_guidance:
        V = eng.V
        x = torch.randn(2 * B, eng.Vp, device=dev) * 3
        ops.logits_guidance(x[:B, :V], x[B:, :V], 1.0, 0.1)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.launches):
                ops.logits_guidance(x[:B, :V], x[B:, :V], 1.0, 0.1)
        graph.replay()
        per = []
        for _ in range(5):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(20):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1) / (20 * args.launches) * 1e3)
        assert bool(torch.isfinite(x[:B, :V]).any())
        print(json.dumps({"launch": "mg_logits_guidance_f32", "pairs": B, "V": V, "launches_per_graph": args.launches,
                          "us_per_launch_in_graph_median": statistics.median(per), "us_per_launch_in_graph_min": min(per),
                          "bytes_read_per_launch": 2 * 2 * B * V * 4, "bytes_written_per_launch": B * V * 4}), flush=True)
