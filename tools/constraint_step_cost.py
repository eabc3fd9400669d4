"""Token step with and without a trie constraint (DESIGN.md "Constrained decoding"): MAGMA_v1, B = 8, prefill 57, 32 tokens.

    python tools/constraint_step_cost.py [--layers 28] [--gen 32] [--steps 3] [--warmup 1] [--out profiles/constraint_step_cost.jsonl]

The captured greedy token step in four cases, interleaved round by round on the same box: (a) plain, (b) a small trie (8 choices),
(c) a large one (12 000 sequences of 3 tokens under a root with 3 000 edges), (d) the four-rule processor launch
(repetition_penalty 1.3, no_repeat_ngram_size 3, min_new_tokens 8, 16 suppress ids) for comparison.  ms per token step =
(generate() of `gen` tokens minus the same call for ONE token) over `gen` - 1 steps, the eos stop switched off -- what a call pays
once (checking the arguments, writing the table: the cases alternate, so every call writes its table again) is `setup_ms`, beside
the plain call's --; and the GPU time of the launch alone by events,
at the root (wide fan-out) and at the two steps behind it (the launch reads no logit: its time does not depend on the values).  One JSON line per case (appended to --out as well)."""
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
    ap.add_argument("--gen", type=int, default=32)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from magma_amd import Magma, ops
    from magma_amd.language_model import GPTJConfig
    from magma_amd.sampling import TokenTrie, trie_forest
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    lm_cfg = GPTJConfig(num_layers=args.layers, vocab_size=50258) if args.layers else None
    model = Magma(args.config, device=dev, lm_config=lm_cfg)
    model.eval()
    eng = model.lm.engine
    B, S, gen = 8, 57, args.gen
    d = model.lm.config.hidden_size
    eos = model.eos_token
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=8, suppress_tokens=list(range(100, 116)))
    ids = [t for t in range(200, 40000) if t != eos]
    small = TokenTrie([[ids[7 * i], ids[7 * i + 1 + i % 3]] for i in range(8)])
    large = TokenTrie([[ids[a], ids[3000 + (a * 4 + j) % 20000], ids[(a + j) % 3000]] for a in range(3000) for j in range(4)])
    g = torch.Generator(device=dev).manual_seed(7)
    emb = torch.randn(B, S, d, device=dev, generator=g).to(torch.bfloat16)
    kw = dict(temperature=0.0, stop_on_eos=False, decode=False)
    cases = [("plain", {}), ("small_trie", dict(constraint=small)), ("large_trie", dict(constraint=large)), ("four_rules", rules)]
    fns = [lambda extra=extra: model.generate(emb, max_steps=gen, **kw, **extra) for _, extra in cases]
    fns += [lambda extra=extra: model.generate(emb, max_steps=1, **kw, **extra) for _, extra in cases]
    for _ in range(args.warmup):
        for fn in fns:
            fn()
    total = [0.0] * len(fns)
    for _ in range(args.steps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            total[i] += time.perf_counter() - t0
    secs = [t / args.steps for t in total]
    n = len(cases)
    step_ms = [(secs[i] - secs[n + i]) / (gen - 1) * 1e3 for i in range(n)]
    setup_ms = [(secs[n + i] - secs[n]) * 1e3 for i in range(n)]

    def ev_time(fn, n=20):
        ts = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return sorted(ts)[len(ts) // 2]

    cache = eng._cache_pool[next(c for c in eng._cache_pool if c[0] == B)]
    logits = cache.decode_state.logits[:, : eng.V]
    launch = {}
    for name, trie in (("small_trie", small), ("large_trie", large)):
        table, roots = trie_forest([trie] * B)
        table, roots, path = table.to(dev), roots.to(dev), ops.trie_path(B, dev)
        hist = torch.tensor([list(trie.sequences[b]) + [eos] * 8 for b in range(B)], dtype=torch.int64, device=dev)
        for step in (0, 1, 2):      # in order, as a loop does: the path cache holds the steps before
            state = torch.tensor([step, -1], dtype=torch.int32, device=dev)
            launch[name, step] = ev_time(lambda: ops.logits_process_constrained(logits, state, hist, table, roots, path, eos=eos))
    state = torch.tensor([gen - 1, -1], dtype=torch.int32, device=dev)
    sup = torch.arange(100, 116, dtype=torch.int32, device=dev)
    launch["four_rules", 0] = ev_time(lambda: ops.logits_process(logits, state, cache.history, repetition_penalty=1.3,
                                                                 no_repeat_ngram_size=3, min_new_tokens=8, eos=eos, suppress=sup))
    lines = []
    for (name, extra), ms, setup in zip(cases, step_ms, setup_ms):
        line = {"config": args.config, "layers": model.lm.config.num_layers, "case": name, "B": B, "gen": gen,
                "one_token_ms": round(secs[n] * 1e3, 3), "setup_ms": round(setup, 3), "step_ms": round(ms, 4), "added_us_per_step": round((ms - step_ms[0]) * 1e3, 2),
                "over_plain": round(ms / step_ms[0], 4)}
        if "constraint" in extra:
            t = extra["constraint"]
            line.update(sequences=len(t.sequences), nodes=t.n_nodes, root_edges=t.first[1], table_ints=int(t.flat().numel()),
                        launch_us={f"step{k}": round(launch[name, k] * 1e3, 2) for k in (0, 1, 2)})
        if name == "four_rules":
            line["launch_us"] = {"last_step": round(launch[name, 0] * 1e3, 2)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
