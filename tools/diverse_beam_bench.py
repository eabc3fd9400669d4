"""Token step of diverse beam search against plain beam search on the same build (DESIGN.md "Diverse beam search"): MAGMA_v1,
B = 2, prompt 57, num_beams = 4 (8 rows: the captured weight-streaming step), 32 steps.

    python tools/diverse_beam_bench.py [--layers 28] [--gen 32] [--rounds 5] [--groups 2] [--penalty 0.5] [--out FILE]

After one warm-up of every leg the rounds run interleaved (prefill, plain, grouped, prefill, plain, grouped, ...), each a whole
generate() call between two device synchronisations; a leg's step time is (call - prefill) / (gen - 1) with the prefill of the
same round.  eos is a token the random model does not favour and early_stopping="never" with length_penalty=0 keeps every
call running all `gen` steps.  The bookkeeping launch alone is timed by device events on the state the last call left.  One
JSON line: every round's step times, their median and spread (max - min), so that a difference can be weighed against the
run-to-run spread.  On a build without num_beam_groups the grouped leg is left out (the plain leg of an older commit)."""
import argparse
import inspect
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--penalty", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from magma_amd import Magma, ops
    from magma_amd.language_model import GPTJConfig
    from magma_amd.sampling import generate
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    lm_cfg = GPTJConfig(num_layers=args.layers, vocab_size=50258) if args.layers else None
    model = Magma(args.config, device=dev, lm_config=lm_cfg)
    model.eval()
    eng = model.lm.engine
    S, gen, B, k = 57, args.gen, args.batch, args.beams
    grouped = "num_beam_groups" in inspect.signature(generate).parameters
    g = torch.Generator(device=dev).manual_seed(7)
    emb = torch.randn(B, S, model.lm.config.hidden_size, device=dev, generator=g).to(torch.bfloat16)
    emb_r = emb.repeat_interleave(k, dim=0)
    common = dict(max_steps=gen, num_beams=k, decode=False, early_stopping="never", length_penalty=0.0)
    legs = {"prefill": lambda: model.lm(inputs_embeds=emb_r, use_cache=True, cache_hint=gen, reuse_cache=True,
                                        eos_token=model.eos_token),
            "plain": lambda: model.generate(emb, **common)}
    if grouped:
        legs["grouped"] = lambda: model.generate(emb, num_beam_groups=args.groups, diversity_penalty=args.penalty, **common)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):                       # warm-up: allocations, first-use packing, the captured step of every leg
        for fn in legs.values():
            timed(fn)
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    steps = {name: [round((t - p) / (gen - 1), 4) for t, p in zip(ms[name], ms["prefill"])] for name in legs if name != "prefill"}

    def summary(v):
        s = sorted(v)
        return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "spread": round(s[-1] - s[0], 4)}

    # the bookkeeping launch alone, on the buffers a call of that leg armed (device events; the state restored between runs)
    def bookkeeping_ms(leg, n=20):
        legs[leg]()
        cache = eng._cache_pool[next(c for c in eng._cache_pool if c[0] == B * k)]
        bm = cache.beam
        saved = {name: t.clone() for name, t in bm.bufs.items() if name != "hist"}
        state0 = cache.sample_state.clone()
        tail = (eng.V, cache.eos, 0.0, "never", gen, cache.sample_state, bm.bufs)
        if leg == "grouped":
            fn = lambda: ops.beam_finish_groups(bm.cand_score, bm.cand_tok, bm.B, k, args.groups, args.penalty, *tail)  # noqa: E731
        else:
            fn = lambda: ops.beam_finish(bm.cand_score, bm.cand_tok, bm.B, k, *tail)  # noqa: E731
        ts = []
        for _ in range(n):
            for name, t in saved.items():
                bm.bufs[name].copy_(t)
            cache.sample_state.copy_(state0)
            cache.sample_state[1] = -1
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return round(sorted(ts)[len(ts) // 2], 4)

    book = {f"{leg}_bookkeeping_ms": bookkeeping_ms(leg) for leg in steps}
    line = {"config": args.config, "layers": model.lm.config.num_layers, "B": B, "num_beams": k, "prompt": S, "gen": gen,
            "rounds": args.rounds, "groups": args.groups if grouped else None, "penalty": args.penalty if grouped else None,
            "prefill_ms": summary([round(t, 3) for t in ms["prefill"]]),
            "step_ms": {name: dict(summary(v), rounds=v) for name, v in steps.items()}, **book}
    if grouped:
        line["grouped_over_plain"] = round(line["step_ms"]["grouped"]["median"] / line["step_ms"]["plain"]["median"], 4)
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
