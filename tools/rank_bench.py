"""Ranking a closed set of answers: Magma.rank (one prefill, one tree forward per group of choices) against Magma.score over the
same candidates (one cache-less forward row per candidate, in batches).  MAGMA_v1, random weights, B = 1, the benchmark's
57-row prompt, choices of 1 to 4 tokens (+ eos) that share first tokens as an answer vocabulary does.

    python tools/rank_bench.py [--layers 28] [--choices 32,2048] [--rounds 3] [--out profiles/rank_bench.jsonl]

After one warm-up of both legs the rounds run interleaved (rank, score, rank, score, ...), each timed with device events around
the whole call; one JSON line per case is printed and appended to --out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_choices(n, vocab, eos, seed):
    """n distinct sequences of 1 to 4 ids; first tokens from a pool of n / 8, so that the trie shares its upper levels."""
    import torch
    g = torch.Generator().manual_seed(seed)
    pool = [t for t in torch.randperm(vocab, generator=g).tolist() if t != eos]
    first, rest = pool[: max(4, n // 8)], pool[max(4, n // 8): max(4, n // 8) + 512]
    seen, out = set(), []
    while len(out) < n:
        ln = int(torch.randint(1, 5, (1,), generator=g))
        q = (first[int(torch.randint(0, len(first), (1,), generator=g))],) + tuple(
            rest[int(torch.randint(0, len(rest), (1,), generator=g))] for _ in range(ln - 1))
        if q not in seen:
            seen.add(q)
            out.append(list(q))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="MAGMA_v1")
    ap.add_argument("--layers", type=int, default=None, help="GPT-J blocks (default: the config's 28)")
    ap.add_argument("--prompt", type=int, default=57)
    ap.add_argument("--choices", default="32,2048")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--score-batch", type=int, default=256, help="candidates per Magma.score call")
    ap.add_argument("--out", default=os.path.join("profiles", "rank_bench.jsonl"))
    args = ap.parse_args()

    import torch
    from magma_amd import Magma
    from magma_amd.language_model import GPTJConfig
    from magma_amd.sampling import TokenTrie, rank_groups
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    lm_cfg = GPTJConfig(num_layers=args.layers, vocab_size=50258) if args.layers else None
    model = Magma(args.config, device=dev, lm_config=lm_cfg)
    model.eval()
    d, eos, V = model.lm.config.hidden_size, model.eos_token, model.lm.engine.V
    g = torch.Generator(device=dev).manual_seed(7)
    prompt = (torch.randn(1, args.prompt, d, device=dev, generator=g) * 0.5).to(torch.bfloat16)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    for n in [int(v) for v in args.choices.split(",")]:
        seqs = make_choices(n, V, eos, seed=n)
        trie = TokenTrie(seqs)
        budget = model.lm.config.max_position_embeddings - args.prompt
        groups = rank_groups(trie, budget)

        def run_rank():
            return model.rank(prompt, trie).logprobs[0]

        def run_score():
            sums = []
            for i in range(0, n, args.score_batch):
                part = seqs[i: i + args.score_batch]
                sc = model.score(prompt.expand(len(part), -1, -1), [q + [eos] for q in part])
                sums.append(sc.logprobs.sum(1))
            return torch.cat(sums)

        _, r0 = timed(run_rank)                   # warm-up of both legs (allocations, first-use packing)
        _, s0 = timed(run_score)
        legs = {"rank_ms": [], "score_ms": []}
        for _ in range(args.rounds):
            legs["rank_ms"].append(round(timed(run_rank)[0], 3))
            legs["score_ms"].append(round(timed(run_score)[0], 3))
        best = {k: min(v) for k, v in legs.items()}
        line = {"config": args.config, "layers": model.lm.config.num_layers, "prompt_rows": args.prompt, "choices": n,
                "trie_nodes": trie.n_nodes - 1, "tree_forwards": len(groups), "candidate_rows_of_score": sum(len(q) for q in seqs),
                "legs": legs, "best_ms": best, "score_over_rank": round(best["score_ms"] / best["rank_ms"], 2),
                "max_abs_diff_of_sums": round(float((r0.double() - s0.double()).abs().max()), 5),
                "same_argmax": int(torch.argmax(r0)) == int(torch.argmax(s0))}
        print(json.dumps(line), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
