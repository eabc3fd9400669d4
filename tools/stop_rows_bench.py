"""Per-row stopping at the bench shape, in ONE process: MAGMA_v1, 28 blocks, B = 8, prefill 57.

  python tools/stop_rows_bench.py [--layers 28] [--steps 250] [--reps 5] [--gen 64] [--out profiles/stop_rows_bench.jsonl]

(a) The captured token step with the default bookkeeping launch (mg_sample_finish) -- measured twice, "default" and "default_again",
    to show the run-to-run spread of one and the same step -- and with per-row stopping armed (mg_sample_finish_rows in its
    place): one eos id, and 8 eos ids + 16 sequences of 16 tokens.  The table holds ids the rows do not emit, so that every row
    stays unfinished and is tested against every item at every step.  Device events around ``--steps`` replays of the captured
    step, every variant on its own cache, the variants' windows interleaved, ``--reps`` windows each; min and median are reported.
(b) One generate() call of ``--gen`` steps whose rows finish at spread-out steps, by stop sequences taken from the plain run's
    own rows: steps run on the device and wall time with and without them (best of five calls after two warm-up calls)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magma_amd import Magma  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="MAGMA_v1")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--layers", type=int, default=0, help="0 = the config's depth (28)")
ap.add_argument("--steps", type=int, default=250)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--gen", type=int, default=64)
ap.add_argument("--out", default="")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("stop_rows_bench: no GPU -- this tool measures, it does not fall back")
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


e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
with torch.no_grad():
    emb = model.embed([images, prompt])
    S0 = int(emb.shape[1])
    eos = model.eos_token

    # ---- (a) the captured token step ----
    plain = model.generate(emb, max_steps=args.gen, temperature=0.0, decode=False, stop_on_eos=False)[:, S0:].cpu()
    unused = [t for t in range(49000, 49400) if not bool((plain == t).any())]
    stops = {"default": None, "rows_1_eos": dict(eos_ids=(unused[0],), stop_seqs=()), "default_again": None,
             "rows_8_eos_16x16": dict(eos_ids=tuple(unused[:8]), stop_seqs=tuple(tuple(unused[8 + j: 24 + j]) for j in range(16)))}
    caches = {}
    for name, stop in stops.items():      # one cache per variant: prefill (arms the bookkeeping), eager step, capture, replay
        o = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=args.steps + 8, eos_token=eos if stop is None else stop["eos_ids"][0],
                     stop=stop)
        cache = o.past_key_values
        for _ in range(3):
            eng.decode(None, cache, stop=stop)
        caches[name] = cache
    ms, finished = {name: [] for name in stops}, {}
    for rep in range(args.reps):              # interleaved windows
        for name, stop in stops.items():
            cache = caches[name]
            cache.pos = S0
            cache.d_pos.fill_(S0)             # the same context length, step counter and (un)finished rows in every window
            cache.sample_state.copy_(torch.tensor([0, -1], dtype=torch.int32))
            if stop is not None:
                cache.finish.copy_(torch.tensor([[-1, 0]] * B, dtype=torch.int32))
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                eng.decode(None, cache, stop=stop)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
            if stop is not None:          # a finished row is no longer tested against the table: reported, so that it shows
                finished[name] = max(finished.get(name, 0), int((cache.finish[:, 0] >= 0).sum()))
    for name in stops:
        emit({"part": "step", "variant": name, "step_ms_min": min(ms[name]), "step_ms_median": statistics.median(ms[name]),
              "step_ms_all": ms[name], "steps_per_window": args.steps, "graphs": len(caches[name].decode_state.graphs),
              "rows_finished_in_a_window": finished.get(name)})
    caches.clear()
    eng._cache_pool.clear()

    # ---- (b) one end-to-end call ----
    rows = plain.tolist()
    seqs = [rows[r][2 + 7 * r: 5 + 7 * r] for r in range(B) if 5 + 7 * r <= args.gen]
    calls = {"default": dict(), "stop_per_row": dict(stop_sequences=seqs)}
    for name, extra in calls.items():
        def call():
            return model.generate(emb, max_steps=args.gen, temperature=0.0, decode=False, return_past_key_values=True,
                                  return_finish=True, **extra)
        for _ in range(2):
            call()
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out, past, fin = call()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        emit({"part": "generate", "variant": name, "max_steps": args.gen, "steps_run": int(past.sample_state[0]),
              "width": int(out.shape[1]) - S0, "kept": fin.kept.tolist(), "reason": fin.reason, "wall_ms_min": min(times) * 1e3,
              "wall_ms_all": [x * 1e3 for x in times]})
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
