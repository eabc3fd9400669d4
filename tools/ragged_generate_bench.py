"""Generate tokens/s of a RAGGED batch (right-padded prompts of different lengths, generate(..., lengths=)) next to the
uniform batch of the same padded shape -- bench.py's headline shape: MAGMA_v1, B = 8, 32 greedy tokens, prefill 57.

    python tools/ragged_generate_bench.py [--layers 28] [--steps 5] [--warmup 2]

Both legs run the same prefill (B x 57 rows, the padding included) and the same captured token step; the ragged one reads
one KV position per row instead of one per batch.  Prints one JSON line."""
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--gen", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    from magma_amd import Magma
    from magma_amd.language_model import GPTJConfig
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    lm_cfg = GPTJConfig(num_layers=args.layers, vocab_size=50258) if args.layers else None
    model = Magma(args.config, device=dev, lm_config=lm_cfg)
    model.eval()
    B, S, gen = args.batch, 57, args.gen
    lengths = [41 + (16 * b) // max(B - 1, 1) for b in range(B)]          # 41 .. 57
    g = torch.Generator(device=dev).manual_seed(7)
    emb = torch.randn(B, S, model.lm.config.hidden_size, device=dev, generator=g).to(torch.bfloat16)
    emb_ragged = emb.clone()
    for b, n in enumerate(lengths):
        emb_ragged[b, n:] = 0

    def leg(e, lens):
        run = lambda: model.generate(e, max_steps=gen, temperature=0.0, decode=False, stop_on_eos=False, lengths=lens)  # noqa: E731
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            run()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        return {"ms_per_generate": round(dt * 1e3, 3), "tokens_per_s": round(B * gen / dt, 1)}

    res = {}
    for rep in range(2):                    # interleaved twice: drift of the box shows as a spread between the two rounds
        res.setdefault("uniform", []).append(leg(emb, None))
        res.setdefault("ragged", []).append(leg(emb_ragged, lengths))
    best = {k: max(r["tokens_per_s"] for r in v) for k, v in res.items()}
    print(json.dumps({"config": args.config, "layers": model.lm.config.num_layers, "batch": B, "gen": gen,
                      "lengths": lengths, "legs": res, "best_tokens_per_s": best,
                      "ragged_over_uniform": round(best["ragged"] / best["uniform"], 4)}))


if __name__ == "__main__":
    main()
