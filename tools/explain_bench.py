"""What explaining an answer costs, in ONE process on the MI355X; writes profiles/explain_bench.jsonl (and prints the lines).

  kernel   mg_attn_prefill_scaled_bf16 beside mg_attn_prefill_bf16 (the unscaled kernel it is built from, MAGMA_ATTN_FWD=5) at
           (B 16, H 16, S 165) and (B 16, H 16, S 2048): device events around ``--launches`` back-to-back launches, the two
           kernels' windows alternating, median and minimum per launch.  A window's time per launch includes the launch gap;
           a kernel time proper comes from rocprofv3 --kernel-trace --stats in a run of its own.
  explain  Magma.explain at 28 blocks, full width: one row, a prompt of 144 image rows + 13 text rows (seeded random embeddings:
           the cost does not depend on their values) and 8 targets, batch_size 16 -- 158 scored rows in 10 forwards of (16, 164).
           Total time (host clock around the call, which ends in a device-to-host copy), and the share of it spent in attention:
           forwards x blocks x the scaled kernel's time per launch at the forward's shape (measured as above) over the total.

  python tools/explain_bench.py [--layers 28] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from magma_amd import Magma, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="MAGMA_v1")
ap.add_argument("--layers", type=int, default=0, help="0 = the config's depth (28)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_bench.jsonl"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("explain_bench: no GPU -- this tool measures, it does not fall back")
dev = torch.device("cuda:0")
os.environ["MAGMA_ATTN_FWD"] = "5"
BF16 = torch.bfloat16
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
lines = []


def emit(rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def kernel_times(B, H, S, launches, reps):
    """ms per launch of (unscaled, scaled), windows alternating."""
    g = torch.Generator().manual_seed(S)
    q = (torch.randn(B, H, S, 256, generator=g) * 0.5).to(BF16).to(dev)
    k = (torch.randn(B, H, S, 256, generator=g) * 0.5).to(BF16).to(dev)
    v = torch.randn(B, H, S, 256, generator=g).to(BF16).to(dev)
    vt = ops.head_transpose(v, B, H, S, sb=H * S * 256, ss=256, sh=S * 256)
    out = torch.empty(B * S, H * 256, dtype=BF16, device=dev)
    scale = torch.rand(B, S, generator=g).to(dev)
    arms = {"mg_attn_prefill_bf16": lambda: ops.attn_prefill(q, k, vt, out, B, H, S),
            "mg_attn_prefill_scaled_bf16": lambda: ops.attn_prefill_scaled(q, k, vt, out, B, H, S, scale)}
    times = {a: [] for a in arms}
    for f in arms.values():
        for _ in range(3):
            f()
    for _ in range(reps):
        for a, f in arms.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[a].append(e0.elapsed_time(e1) / launches)
    return times


with torch.no_grad():
    for S in (165, 2048):
        t = kernel_times(16, 16, S, args.launches, args.reps)
        base, sc = t["mg_attn_prefill_bf16"], t["mg_attn_prefill_scaled_bf16"]
        emit({"what": "kernel", "B": 16, "H": 16, "S": S, "launches_per_window": args.launches,
              "unscaled_ms_median": statistics.median(base), "unscaled_ms_min": min(base),
              "scaled_ms_median": statistics.median(sc), "scaled_ms_min": min(sc),
              "scaled_over_unscaled_median": statistics.median(sc) / statistics.median(base), "unscaled_ms_all": base, "scaled_ms_all": sc})

    torch.manual_seed(1234)
    kw = {}
    if args.layers:
        from magma_amd.language_model import GPTJConfig
        kw["lm_config"] = GPTJConfig(num_layers=args.layers, vocab_size=50258)
    model = Magma(args.config, device=dev, **kw)
    model.eval()
    eng = model.lm.engine
    g = torch.Generator().manual_seed(2)
    n_prompt, n_tgt, bs = 144 + 13, 8, 16
    prompt = (torch.randn(1, n_prompt, eng.d, generator=g) * 0.5).to(BF16).to(dev)
    targets = torch.randint(0, 50256, (1, n_tgt), generator=g)
    W = n_prompt + n_tgt - 1
    model.explain(prompt, targets, batch_size=bs)            # warm-up: every shape of the timed call
    total = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ex = model.explain(prompt, targets, batch_size=bs)
        torch.cuda.synchronize()
        total.append((time.perf_counter() - t0) * 1e3)
    n_fwd = -(-(1 + n_prompt) // bs)
    attn = statistics.median(kernel_times(bs, eng.H, W, args.launches, args.reps)["mg_attn_prefill_scaled_bf16"])
    blocks = len(eng.layers)
    emit({"what": "explain", "blocks": blocks, "d": eng.d, "prompt_rows": n_prompt, "targets": n_tgt, "batch_size": bs,
          "scored_rows": 1 + n_prompt, "forwards": n_fwd, "forward_shape": [bs, W], "total_ms_median": statistics.median(total),
          "total_ms_min": min(total), "total_ms_all": total, "attention_ms_per_launch": attn,
          "attention_share": n_fwd * blocks * attn / statistics.median(total),
          "relevance_finite": bool(torch.isfinite(ex.relevance).all())})

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
