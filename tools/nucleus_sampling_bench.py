"""transformers' sampler at the bench shape, in ONE process: MAGMA_v1, 28 blocks, B = 8, prefill 57.

  python tools/nucleus_sampling_bench.py [--layers 28] [--steps 250] [--reps 5] [--out profiles/nucleus_sampling_bench.jsonl]

(a) The captured token step with the reference's selection launch (mg_sample_f32 at the default call's (0.7, 0, 0.9)) -- measured
    twice, "reference" and "reference_again", to show the run-to-run spread of one and the same step -- and with transformers'
    sampler in its place (mg_sample_warp_f32) at top_p = 0.9, at top_k = 40 with top_p = 0.9, and at min_p = 0.05.  Device events
    around ``--steps`` replays of the captured step, every variant on its own cache, the variants' windows interleaved, ``--reps``
    windows each; min and median are reported, and the ratio of every variant's min to the smaller of the two reference minima.
(b) The selection launch alone on the logits of one token step (eager launches between device events, same interleaving): where a
    difference of (a) comes from.  ``kept`` is the number of tokens each row's filter left."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magma_amd import Magma, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="MAGMA_v1")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--layers", type=int, default=0, help="0 = the config's depth (28)")
ap.add_argument("--steps", type=int, default=250)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("nucleus_sampling_bench: no GPU -- this tool measures, it does not fall back")
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
lines = []


def emit(d):
    lines.append(json.dumps(d))
    print(lines[-1], flush=True)


MODES = {"reference": (0.7, 0, 0.9), "warp_top_p": ("warp", 0.7, 0, 0.9, 0.0), "warp_top_k_top_p": ("warp", 0.7, 40, 0.9, 0.0),
         "warp_min_p": ("warp", 0.7, 0, 0.0, 0.05), "reference_again": (0.7, 0, 0.9)}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
with torch.no_grad():
    emb = model.embed([images, prompt])
    S0 = int(emb.shape[1])

    # ---- (a) the captured token step ----
    caches = {}
    for name, mode in MODES.items():      # one cache per variant: prefill (arms the bookkeeping), eager step, capture, replay
        o = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=args.steps + 8, eos_token=model.eos_token, sampling=mode, seed=7)
        cache = o.past_key_values
        for _ in range(3):
            eng.decode(None, cache, sampling=mode)
        caches[name] = cache
    ms = {name: [] for name in MODES}
    for rep in range(args.reps):              # interleaved windows
        for name, mode in MODES.items():
            cache = caches[name]
            cache.pos = S0
            cache.d_pos.fill_(S0)             # the same context length and step counter in every window
            cache.sample_state.copy_(torch.tensor([0, -1], dtype=torch.int32))
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                eng.decode(None, cache, sampling=mode)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
    base = min(min(ms["reference"]), min(ms["reference_again"]))
    for name, mode in MODES.items():
        emit({"part": "step", "variant": name, "mode": list(mode), "step_ms_min": min(ms[name]),
              "step_ms_median": statistics.median(ms[name]), "step_ms_all": ms[name], "ratio_to_reference_min": min(ms[name]) / base,
              "steps_per_window": args.steps, "graphs": len(caches[name].decode_state.graphs)})

    # ---- (b) the selection launch alone ----
    cache = caches["reference"]
    logits = cache.decode_state.logits[:, : eng.V].clone()
    state = torch.tensor([3, -1], dtype=torch.int32, device=dev)
    tok, f = torch.empty(B, dtype=torch.int64, device=dev), torch.empty_like(logits)

    def launch(mode, **k):
        if mode[0] == "warp":
            return ops.sample_warp(logits, mode[1], mode[2], mode[3], mode[4], cache.seed, state, out=tok, **k)
        return ops.sample(logits, mode[0], mode[1], mode[2], cache.seed, state, out=tok, **k)

    us, kept = {name: [] for name in MODES}, {}
    for name, mode in MODES.items():
        launch(mode, filtered=f)
        kept[name] = (~torch.isneginf(f)).sum(1).tolist()
    for rep in range(args.reps):
        for name, mode in MODES.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                launch(mode)
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) / args.steps * 1e3)
    for name, mode in MODES.items():
        emit({"part": "launch", "variant": name, "mode": list(mode), "launch_us_min": min(us[name]),
              "launch_us_median": statistics.median(us[name]), "launch_us_all": us[name], "kept": kept[name]})
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
