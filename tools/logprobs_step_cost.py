"""What token log-probabilities cost per captured token step (DESIGN.md "Token log-probabilities"): MAGMA_v1, 28 blocks, B = 8,
greedy, the step with the mode off, with return_logprobs (no alternatives) and with top_logprobs = 5, in ONE process.

  python tools/logprobs_step_cost.py [--steps 250] [--reps 4] [--layers 0]

The method of tools/decode_w4_bench.py: every mode has its own armed cache (prefill, eager step, capture), device events around
``--steps`` replays of its captured feed-back step, best of ``--reps`` windows, the windows of the modes alternating; every window
starts at the same context length and at step 0 (so that the launch writes its column: past the buffers it writes nothing)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magma_amd import Magma  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="MAGMA_v1")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--steps", type=int, default=250)
ap.add_argument("--layers", type=int, default=0, help="0 = the config's depth (28)")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("logprobs_step_cost: no GPU -- this tool measures, it does not fall back")
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
MODES = {"off": None, "logprobs": 0, "top5": 5}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
zero = torch.tensor([0, -1], dtype=torch.int32, device=dev)
with torch.no_grad():
    emb = model.embed([images, prompt])
    S0 = int(emb.shape[1])
    caches, ms = {}, {m: [] for m in MODES}
    for m, n_top in MODES.items():
        kw = {} if n_top is None else {"logprobs": n_top}
        out = model.lm(inputs_embeds=emb, use_cache=True, cache_hint=args.steps + 8, eos_token=model.eos_token, **kw)
        caches[m] = out.past_key_values
        for _ in range(3):
            eng.decode(None, caches[m], **kw)
    for rep in range(args.reps):
        for m, n_top in MODES.items():
            cache = caches[m]
            kw = {} if n_top is None else {"logprobs": n_top}
            cache.pos = S0
            cache.d_pos.fill_(S0)
            cache.sample_state.copy_(zero)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                eng.decode(None, cache, **kw)
            e1.record()
            torch.cuda.synchronize()
            ms[m].append(e0.elapsed_time(e1) / args.steps)
    graphs = {m: len(c.decode_state.graphs) for m, c in caches.items()}
print(json.dumps({"batch": B, "layers": len(eng.layers), "steps": args.steps, "graphs": graphs,
                  "step_ms": {m: min(v) for m, v in ms.items()}, "step_ms_all": ms}))
