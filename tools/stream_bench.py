"""Request streams at the bench shape, in ONE process: MAGMA_v1, 28 blocks, 8 slots, 64 requests with a 57-row prompt.

  python tools/stream_bench.py [--layers 28] [--requests 64] [--steps 250] [--reps 5] [--out FILE (default profiles/stream_bench.jsonl)]

(a) Tokens that count per second over the same 64 requests, whose max_new_tokens come from a fixed list spread over 5 to 40 (eos
    is an id outside the tokenizer's range, so every request runs to its own limit unless the model happens to emit it):
    ``generate_stream`` with 8 slots; static ``generate(stop_per_row=True)`` batches of 8 in the requests' order, each with its
    own largest limit as ``max_steps``; the static leg again, to show the spread.  One warm-up pass of every leg first.  The
    session is given ``max_prompt`` = the prompt length, 57: every admission prefill then runs over (8, 64) rows.
(b) The captured token step with the slot bookkeeping (mg_sample_finish_slots) against the per-row one (mg_sample_finish_rows),
    measured as tools/stop_rows_bench.py measures: device events around ``--steps`` replays, windows interleaved, the same
    context length in every window, ``--reps`` windows each; the per-row step twice, to show the spread.

  python tools/stream_bench.py --prefix-rows 656 [--request-rows 160] [--out FILE (default profiles/stream_prefix_bench.jsonl)]

The session prefix (DESIGN.md "Request streams", session prefix) instead: 64 requests of ``--request-rows`` rows behind ONE prefix
of ``--prefix-rows`` rows, max_new_tokens spread over 3 to 12, eos disabled -- few-shot evaluation.
(a) Tokens that count per second and the rows prefilled in total, legs interleaved after one warm-up pass of each, wall time
    around each leg ending in a device synchronise: ``generate_stream(prefix=...)``; ``generate_stream`` on the concatenated
    prompts (``max_prompt`` = prefix + request rows); static ``generate(past_key_values=cache.expand(8), stop_per_row=True)`` in
    batches of 8 behind one ``cache_prompt``.
(b) The captured token step of a session with the prefix against the same session without it at equal own-context length: the
    cost of the P more positions per row the decode attention reads.  Medians over interleaved windows of ``--steps`` replays.
  python tools/stream_bench.py --choices [--prefix-rows 656] [--request-rows 160] [--out FILE (default profiles/choose_stream_bench.jsonl)]

Choosing over a request stream (DESIGN.md "Choosing over a request stream"): 64 requests of ``--request-rows`` rows behind ONE prefix
(default 656 rows), every request with an answer set of its own -- four choices whose lengths are spread over 1 to 12 tokens --.
(a) Answers per second, legs interleaved after one warm-up pass of each: ``choose_stream(prefix=...)``; the same with
    ``share_prefix=True``; static ``choose(past_key_values=cache.expand(8))`` in batches of 8 behind one ``cache_prompt``.
(b) The captured slot step with the constraint and log-probability launches against the slot step without them and against
    generate()'s per-row step with them: device events around windows of min(``--steps``, 48) replays, interleaved, medians of
    ``--reps``.  Every row walks a trie of ONE 64-token sequence, so no row finishes inside a window (a finished slot stops
    advancing and would make its step cheaper): every record carries ``rows_finished``, which must be 0, and every window of every
    variant starts from the same positions.

  python tools/stream_bench.py --prefix-rows 656 --share-prefix [--out FILE (default profiles/stream_shared_prefix_bench.jsonl)]

The shared session prefix (DESIGN.md "Shared session prefix") against the per-slot copies, in the same process: the throughput
legs become ``generate_stream(prefix=..., share_prefix=True)`` and ``generate_stream(prefix=...)``, interleaved; the step part
gains the variant ``with_shared_prefix`` (every step record carries the live-cache bytes), and one more record times the
prefix-partials launch alone (one per block, captured, replayed).

  python tools/stream_bench.py --per-request [--out FILE (default profiles/stream_per_request_bench.jsonl)]

Per-request sampling (DESIGN.md "Per-request sampling"): the captured step of an 8-slot session sampled at temperature 0.7, top_k 40,
once under the session-wide sampler (mg_sample_f32: one set of launch arguments, one seed) and once under the per-row launch
(mg_sample_rows_f32: the same settings in every row's record of the device table, eight seeds).  Device events around ``--steps``
replays, windows interleaved, every window from the same positions, medians of ``--reps``; the session-wide step runs twice
(``session_wide``, ``session_wide_again``): the difference of the two is the spread the per-row step is read against.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magma_amd import Magma  # noqa: E402
from magma_amd.engine import LMEngine, SlotSession  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="MAGMA_v1")
ap.add_argument("--layers", type=int, default=0, help="0 = the config's depth (28)")
ap.add_argument("--slots", type=int, default=8)
ap.add_argument("--requests", type=int, default=64)
ap.add_argument("--every", type=int, default=0, help="0 = MAGMA_EOS_CHECK_EVERY (8)")
ap.add_argument("--steps", type=int, default=250)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--prefix-rows", type=int, default=0, help="P > 0: measure the session prefix instead (see the module docstring)")
ap.add_argument("--share-prefix", action="store_true", help="with --prefix-rows: add the share_prefix=True legs (one copy of the "
                "prefix, read once per step for all rows), the prefix-partials launch alone and the live-cache bytes")
ap.add_argument("--choices", action="store_true", help="measure choose_stream instead (see the module docstring)")
ap.add_argument("--per-request", action="store_true", help="measure the per-row sampling launch against the session-wide one "
                "(see the module docstring)")
ap.add_argument("--request-rows", type=int, default=160, help="rows of every request in the --prefix-rows mode")
ap.add_argument("--out", default=None, help="default: profiles/stream_bench.jsonl, profiles/stream_prefix_bench.jsonl with --prefix-rows")
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                            "stream_per_request_bench.jsonl" if args.per_request else
                            "choose_stream_bench.jsonl" if args.choices else
                            "stream_shared_prefix_bench.jsonl" if args.prefix_rows and args.share_prefix else
                            "stream_prefix_bench.jsonl" if args.prefix_rows else "stream_bench.jsonl")
if args.choices and not args.prefix_rows:
    args.prefix_rows = 656
if args.share_prefix and not args.prefix_rows:
    sys.exit("stream_bench: --share-prefix needs --prefix-rows")

if not torch.cuda.is_available():
    sys.exit("stream_bench: no GPU -- this tool measures, it does not fall back")
dev = torch.device("cuda:0")
torch.manual_seed(1234)
kw = {}
if args.layers:
    from magma_amd.language_model import GPTJConfig
    kw["lm_config"] = GPTJConfig(num_layers=args.layers, vocab_size=50258)
model = Magma(args.config, device=dev, **kw)
model.eval()
eng = model.lm.engine
B = args.slots
g = torch.Generator(device=dev).manual_seed(1)
images = torch.randn(8, 3, 224, 224, device=dev, generator=g).to(torch.bfloat16)
prompt = torch.randint(0, 50256, (8, 8), device=dev, generator=g)
LIMITS = [5 + (23 * i) % 36 for i in range(args.requests)]         # 5 .. 40, every residue of 36 in turn
EOS = 50257
lines = []


def emit(d):
    lines.append(json.dumps(d))
    print(lines[-1], flush=True)




def write_out():
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def choices_mode():
    """--choices: answers per second of choose_stream against static choose batches, and the slot step with the constraint and
    log-probability launches against the step without them and against generate()'s per-row step with them."""
    from magma_amd.sampling import TokenTrie
    P, R, n_top = args.prefix_rows, args.request_rows, 3
    emb = model.embed([images, torch.randint(0, 50256, (8, R - 49), device=dev, generator=g)])
    assert emb.shape[1] == R, emb.shape
    prefix = eng.embed_ids(torch.randint(0, 50256, (1, P), device=dev, generator=g))[0]
    host = torch.Generator().manual_seed(7)

    def answer_set(i):             # four choices, lengths spread over 1 .. 12: the longest of request i is 1 + (5 i) % 12
        top = 1 + (5 * i) % 12
        lens = sorted({top, max(1, top // 2), max(1, top // 3), 1})
        return [torch.randint(0, 50256, (n,), generator=host).tolist() for n in lens]

    sets = [answer_set(i) for i in range(args.requests)]
    tries = [TokenTrie(c) for c in sets]
    requests = [(emb[i % 8], tries[i]) for i in range(args.requests)]
    longest = max(t.max_len() for t in tries)
    skw = dict(slots=B, max_choice_tokens=longest, max_prompt=R, eos_token=[EOS], top_logprobs=n_top, every=args.every or None)

    def leg_stream(share=False):
        return sum(int(r.tokens.numel()) for r in model.choose_stream(requests, prefix=prefix, share_prefix=share, **skw))

    def leg_static():
        cache, n = model.cache_prompt(prefix[None]), 0
        for i in range(0, args.requests, B):
            group = requests[i:i + B]
            _, lp = model.choose(torch.stack([x[0] for x in group]), [x[1] for x in group], past_key_values=cache.expand(len(group)),
                                 eos_token=[EOS], top_logprobs=n_top, eos_check_every=args.every or None)
            n += int(lp.count.sum())
        return n

    legs = [("choose_stream_prefix", leg_stream), ("choose_stream_shared_prefix", lambda: leg_stream(True)), ("static_choose_expand", leg_static)]
    for _, leg in legs:
        leg()
    for rep in range(args.reps):
        for name, leg in legs:
            torch.cuda.synchronize()
            t = time.perf_counter()
            n = leg()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            emit({"part": "throughput", "leg": name, "rep": rep, "requests": args.requests, "slots": B, "prefix_rows": P, "request_rows": R,
                  "answer_tokens": n, "wall_s": dt, "answers_per_s": args.requests / dt, "longest_choice": longest})
    for name, _ in legs:
        runs = [x for x in map(json.loads, lines) if x["part"] == "throughput" and x["leg"] == name]
        emit({"part": "throughput_median", "leg": name, "answers_per_s_median": statistics.median(x["answers_per_s"] for x in runs),
              "wall_s_median": statistics.median(x["wall_s"] for x in runs), "answer_tokens": runs[0]["answer_tokens"]})
    eng._cache_pool.clear()

    # ---- the captured step: slots with the modes, slots without, generate()'s per-row step with the modes ----
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stop = dict(eos_ids=(EOS,), stop_seqs=())
    steps = min(args.steps, 48)
    n_new = steps + 8
    walks = [TokenTrie([torch.randint(0, 50256, (64,), generator=host).tolist()]) for _ in range(B)]      # one path: nobody finishes
    plans = {"slots_constraint_logprobs": LMEngine.selection_plan(stop=stop, vocab=eng.V, slots=True, constraint=True, logprobs=n_top),
             "slots_plain": LMEngine.selection_plan(stop=stop, vocab=eng.V, slots=True)}
    held = {}
    for name, plan in plans.items():
        ses = SlotSession(eng, plan, slots=B, max_new=n_new, max_prompt=R, every=1, admit_rows=B)
        ses._admit([(i, emb[i % 8], n_new) + ((walks[i],) if plan.cons is not None else ()) for i in range(B)], list(range(B)))
        sc = ses.cache
        tensors = (sc.d_pos, sc.finish, sc.slot_table, sc.sample_state, ses.st.token)
        held[name] = (ses, tensors, [t.clone() for t in tensors], list(ses.occ))
        for _ in range(3):
            ses._step()
    rows_kw = dict(plan=LMEngine.selection_plan(stop=stop, constraint=walks, logprobs=n_top, vocab=eng.V))      # built once
    o = model.lm(inputs_embeds=emb[:B] if B <= 8 else emb.repeat(2, 1, 1)[:B], use_cache=True, cache_hint=n_new, eos_token=EOS,
                 lengths=[R] * B, **rows_kw)
    rows_cache = o.past_key_values
    for _ in range(3):
        eng.decode(None, rows_cache, **rows_kw)
    ms = {"slots_constraint_logprobs": [], "slots_plain": [], "rows_constraint_logprobs": []}
    finished = dict.fromkeys(ms, 0)
    for rep in range(args.reps):
        for name in ms:
            if name in held:
                ses, tensors, keep, occ = held[name]
                for t, k in zip(tensors, keep):
                    t.copy_(k)
                ses.steps, ses.occ = 0, list(occ)
                run, fin = ses._step, ses.cache.finish
            else:               # step 0 again: the walk starts at the root, the step writes its own history
                rows_cache.pos = R
                rows_cache.d_pos.fill_(R)
                rows_cache.sample_state.copy_(torch.tensor([0, -1], dtype=torch.int32))
                rows_cache.finish.copy_(torch.tensor([[-1, 0]] * B, dtype=torch.int32))
                run, fin = (lambda: eng.decode(None, rows_cache, **rows_kw)), rows_cache.finish  # noqa: E731
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / steps)
            finished[name] = max(finished[name], int((fin[:, 0] >= 0).sum()))
    for name in ms:
        emit({"part": "step", "variant": name, "own_rows": R, "step_ms_min": min(ms[name]), "step_ms_median": statistics.median(ms[name]),
              "step_ms_all": ms[name], "steps_per_window": steps, "rows_finished": finished[name]})
    write_out()


def prefix_mode():
    """--prefix-rows P: the three throughput legs and the step with and without the prefix."""
    P, R = args.prefix_rows, args.request_rows
    limits = [3 + (7 * i) % 10 for i in range(args.requests)]           # 3 .. 12, every residue of 10 in turn
    emb = model.embed([images, torch.randint(0, 50256, (8, R - 49), device=dev, generator=g)])       # 49 image rows + text
    assert emb.shape[1] == R, emb.shape
    prefix = eng.embed_ids(torch.randint(0, 50256, (1, P), device=dev, generator=g))[0]
    requests = [(emb[i % 8], limits[i]) for i in range(args.requests)]
    joined = [(torch.cat([prefix, e]), n) for e, n in requests]
    admit, passes = SlotSession._admit, []

    def counted(self, batch, slots):
        passes.append(self.n_admit * self.S_stage)
        admit(self, batch, slots)

    SlotSession._admit = counted
    skw = dict(slots=B, max_new_tokens=max(limits), eos_token=[EOS], decode=False, every=args.every or None)

    def leg_prefix():
        n = sum(int(r.tokens.numel()) for r in model.generate_stream(requests, max_prompt=R, prefix=prefix, **skw))
        return n, P + sum(passes)

    def leg_shared():
        n = sum(int(r.tokens.numel()) for r in model.generate_stream(requests, max_prompt=R, prefix=prefix, share_prefix=True, **skw))
        return n, P + sum(passes)

    def leg_joined():
        n = sum(int(r.tokens.numel()) for r in model.generate_stream(joined, max_prompt=P + R, **skw))
        return n, sum(passes)

    def leg_static():
        cache, n, rows = model.cache_prompt(prefix[None]), 0, P
        for i in range(0, args.requests, B):
            group = requests[i:i + B]
            lim = torch.tensor([x[1] for x in group])
            out, fin = model.generate(torch.stack([x[0] for x in group]), past_key_values=cache.expand(len(group)), max_steps=int(lim.max()),
                                      temperature=0.0, decode=False, eos_token=[EOS], stop_per_row=True, return_finish=True,
                                      eos_check_every=args.every or None)
            n += int(torch.minimum(fin.kept, lim).sum())
            rows += len(group) * R
        return n, rows

    legs = [("generate_stream_prefix", leg_prefix), ("generate_stream_concatenated", leg_joined), ("static_expand", leg_static)]
    if args.share_prefix:           # interleaved with the unshared leg, which is its yardstick
        legs = [("generate_stream_shared_prefix", leg_shared), ("generate_stream_prefix", leg_prefix)]
    for _, leg in legs:             # one warm-up pass of every leg
        leg()
    for rep in range(args.reps):
        for name, leg in legs:
            passes.clear()
            torch.cuda.synchronize()
            t = time.perf_counter()
            n, rows = leg()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            emit({"part": "throughput", "leg": name, "rep": rep, "requests": args.requests, "slots": B, "prefix_rows": P, "request_rows": R,
                  "tokens_that_count": n, "wall_s": dt, "tokens_per_s": n / dt, "rows_prefilled": rows, "limits_sum": sum(limits)})
    for name, _ in legs:
        runs = [json.loads(x) for x in lines]
        runs = [x for x in runs if x["part"] == "throughput" and x["leg"] == name]
        emit({"part": "throughput_median", "leg": name, "tokens_per_s_median": statistics.median(x["tokens_per_s"] for x in runs),
              "wall_s_median": statistics.median(x["wall_s"] for x in runs), "rows_prefilled": runs[0]["rows_prefilled"],
              "tokens_that_count": runs[0]["tokens_that_count"]})
    SlotSession._admit = admit
    eng._cache_pool.clear()

    # ---- the captured token step with and without the prefix, at the same own-context length ----
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    plan = LMEngine.selection_plan(stop=dict(eos_ids=(EOS,), stop_seqs=()), vocab=eng.V, slots=True)
    held = {}
    variants = [("with_prefix", prefix, False), ("without_prefix", None, False), ("without_prefix_again", None, False)]
    if args.share_prefix:
        variants.insert(0, ("with_shared_prefix", prefix, True))
    for name, given, share in variants:
        ses = SlotSession(eng, plan, slots=B, max_new=args.steps + 8, max_prompt=R, every=1, admit_rows=B, prefix=given, share_prefix=share)
        ses._admit([(i, emb[i % 8], args.steps + 8) for i in range(B)], list(range(B)))
        sc = ses.cache
        tensors = (sc.d_pos, sc.finish, sc.slot_table, sc.sample_state, ses.st.token)
        held[name] = (ses, tensors, [t.clone() for t in tensors], list(ses.occ))
        for _ in range(3):
            ses._step()
    ms = {name: [] for name in held}
    for rep in range(args.reps):
        for name, (ses, tensors, keep, occ) in held.items():
            for t, k in zip(tensors, keep):
                t.copy_(k)
            ses.steps, ses.occ = 0, list(occ)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                ses._step()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
    for name in ms:
        emit({"part": "step", "variant": name, "prefix_rows": held[name][0].P, "own_rows": R, "step_ms_min": min(ms[name]),
              "step_ms_median": statistics.median(ms[name]), "step_ms_all": ms[name], "steps_per_window": args.steps,
              "live_cache_bytes": sum(t.numel() * t.element_size() for t in (held[name][0].cache.k, held[name][0].cache.v)),
              "shared_prefix_bytes": sum(t.numel() * t.element_size() for t in (held[name][0].cache.prefix_k, held[name][0].cache.prefix_v)
                                         if t is not None)})
    if args.share_prefix:           # the prefix-partials launch alone: one per block, captured, replayed
        ses = held["with_shared_prefix"][0]
        graph = torch.cuda.CUDAGraph()
        for li in range(eng.L):
            eng._attn_prefix(ses.cache, ses.st, li)
        with torch.cuda.graph(graph):
            for li in range(eng.L):
                eng._attn_prefix(ses.cache, ses.st, li)
        us = []
        for rep in range(args.reps):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(50):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / 50)
        emit({"part": "prefix_partials_alone", "prefix_rows": P, "slots": B, "blocks": eng.L, "chunks": ses.st.shared[1].shape[2],
              "us_per_step_median": statistics.median(us), "us_per_launch_median": statistics.median(us) / eng.L, "us_per_step_all": us})
    write_out()


def per_request_mode():
    """--per-request: the captured sampled slot step, session-wide sampler against the per-row launch."""
    emb = model.embed([images, prompt])
    S0, n_new = int(emb.shape[1]), args.steps + 8
    stop = dict(eos_ids=(EOS,), stop_seqs=())
    T, K, TOP_P = 0.7, 40, 0.9
    plans = {"session_wide": LMEngine.selection_plan(sampling=(T, K, TOP_P), stop=stop, vocab=eng.V, slots=True),
             "per_row": LMEngine.selection_plan(sampling=("rows", False), stop=stop, vocab=eng.V, slots=True)}
    plans["session_wide_again"] = plans["session_wide"]
    held = {}
    for name, plan in plans.items():
        ses = SlotSession(eng, plan, slots=B, max_new=n_new, max_prompt=S0, every=1, admit_rows=B, seed=5)
        ses._admit([(i, emb[i % 8], n_new) + (((T, K, TOP_P, 0.0, 100 + i),) if plan.is_rows else ()) for i in range(B)], list(range(B)))
        sc = ses.cache
        tensors = (sc.d_pos, sc.finish, sc.slot_table, sc.sample_state, ses.st.token)
        held[name] = (ses, tensors, [t.clone() for t in tensors], list(ses.occ))
        for _ in range(3):
            ses._step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, finished = {name: [] for name in held}, dict.fromkeys(held, 0)
    for rep in range(args.reps):
        for name, (ses, tensors, keep, occ) in held.items():
            for t, k in zip(tensors, keep):
                t.copy_(k)
            ses.steps, ses.occ = 0, list(occ)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                ses._step()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
            finished[name] = max(finished[name], int((ses.cache.finish[:, 0] >= 0).sum()))
    for name in ms:
        emit({"part": "step", "variant": name, "slots": B, "blocks": eng.L, "prompt_rows": S0, "temperature": T, "top_k": K, "top_p": TOP_P,
              "step_ms_min": min(ms[name]), "step_ms_median": statistics.median(ms[name]), "step_ms_all": ms[name],
              "steps_per_window": args.steps, "rows_finished": finished[name]})
    med = {name: statistics.median(v) for name, v in ms.items()}
    emit({"part": "step_summary", "session_wide_ms": med["session_wide"], "per_row_ms": med["per_row"],
          "spread_ms": abs(med["session_wide_again"] - med["session_wide"]), "per_row_minus_session_wide_ms": med["per_row"] - med["session_wide"]})
    write_out()


with torch.no_grad():
    if args.per_request:
        per_request_mode()
        sys.exit(0)
    if args.prefix_rows:
        choices_mode() if args.choices else prefix_mode()
        sys.exit(0)
    emb = model.embed([images, prompt])
    S0 = int(emb.shape[1])
    requests = [(emb[i % 8], LIMITS[i]) for i in range(args.requests)]

    def leg_stream():
        n = 0
        for r in model.generate_stream(requests, slots=B, max_new_tokens=max(LIMITS), max_prompt=S0, eos_token=[EOS], decode=False,
                                       every=args.every or None):
            n += int(r.tokens.numel())
        return n

    def leg_static():
        n = 0
        for i in range(0, args.requests, B):
            group = requests[i:i + B]
            lim = torch.tensor([x[1] for x in group])
            out, fin = model.generate(torch.stack([x[0] for x in group]), max_steps=int(lim.max()), temperature=0.0, decode=False,
                                      eos_token=[EOS], stop_per_row=True, return_finish=True, eos_check_every=args.every or None)
            n += int(torch.minimum(fin.kept, lim).sum())
        return n

    # ---- (a) tokens that count per second ----
    legs = [("generate_stream", leg_stream), ("static", leg_static), ("static_again", leg_static)]
    for _, leg in legs[:2]:         # one warm-up pass of every distinct leg: code objects, the pool's caches, captured steps
        leg()
    for name, leg in legs:
        torch.cuda.synchronize()
        t = time.perf_counter()
        n = leg()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        emit({"part": "throughput", "leg": name, "requests": args.requests, "slots": B, "prompt_rows": S0, "tokens_that_count": n,
              "wall_s": dt, "tokens_per_s": n / dt, "limits_sum": sum(LIMITS)})
    eng._cache_pool.clear()

    # ---- (b) the captured token step ----
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stop = dict(eos_ids=(EOS,), stop_seqs=())
    caches = {}
    for name in ("rows", "rows_again"):
        o = model.lm(inputs_embeds=emb[:B] if B <= 8 else emb.repeat(2, 1, 1)[:B], use_cache=True, cache_hint=args.steps + 8,
                     eos_token=EOS, stop=stop, lengths=[S0] * B)
        caches[name] = o.past_key_values
        for _ in range(3):
            eng.decode(None, caches[name], stop=stop)
    plan = LMEngine.selection_plan(stop=stop, vocab=eng.V, slots=True)
    ses = SlotSession(eng, plan, slots=B, max_new=args.steps + 8, max_prompt=S0, every=1, admit_rows=B)
    ses._admit([(i, emb[i % 8], args.steps + 8) for i in range(B)], list(range(B)))
    sc = ses.cache
    keep = [t.clone() for t in (sc.d_pos, sc.finish, sc.slot_table, sc.sample_state, ses.st.token)]
    occ = list(ses.occ)
    for _ in range(3):
        ses._step()
    ms = {"rows": [], "slots": [], "rows_again": []}
    for rep in range(args.reps):
        for name in ms:
            if name == "slots":
                for t, k in zip((sc.d_pos, sc.finish, sc.slot_table, sc.sample_state, ses.st.token), keep):
                    t.copy_(k)
                ses.steps, ses.occ = 0, list(occ)
                run = ses._step
            else:
                cache = caches[name]
                cache.pos = S0
                cache.d_pos.fill_(S0)
                cache.sample_state.copy_(torch.tensor([0, -1], dtype=torch.int32))
                cache.finish.copy_(torch.tensor([[-1, 0]] * B, dtype=torch.int32))
                run = lambda: eng.decode(None, cache, stop=stop)  # noqa: E731
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
    for name in ms:
        emit({"part": "step", "variant": name, "step_ms_min": min(ms[name]), "step_ms_median": statistics.median(ms[name]),
              "step_ms_all": ms[name], "steps_per_window": args.steps,
              "rows_finished": int(((sc if name == "slots" else caches[name]).finish[:, 0] >= 0).sum())})
write_out()
