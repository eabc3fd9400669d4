"""Token selection of the HIP engine: a step's checked selection modes (SelectionPlan, StepKey, ConstraintMode), the device state
of beam and contrastive search (BeamBuffers, ContrastBuffers), and TokenSelection, the base class of engine.LMEngine that turns a
step's logits into its token.  Nothing here touches a weight or imports the engine: ``KVCache`` and ``LMOutput`` appear in
annotations only.  ``ops`` is called through the module, so that tests/launch_trace.py sees every launch made here."""
from __future__ import annotations

from typing import Any, NamedTuple, Optional

import torch

from . import ops

BF16 = torch.bfloat16


class BeamBuffers:
    """Device state of beam search over a KV cache of R = B * k rows (DESIGN.md "Beam search"): running scores, the k finished
    slots per sample (scores, flags, lengths, tokens), the early-stop latch per sample, the parent map and the per-row top-2k
    candidates of a step, staging copies of the token rows, and K / V staging buffers for the cache reorder.  With G > 1 groups
    (DESIGN.md "Diverse beam search") every group of k / G rows is a sample of its own: B * G latches, running scores
    [0, -1e9, ...] per group, and candidate lists of k + k / G entries per row."""

    def __init__(self, cache: KVCache, k: int, token: torch.Tensor, G: int = 1):
        R, dev = cache.B, cache.k.device
        assert R % k == 0 and k % G == 0
        self.k, self.B, self.G = k, R // k, G
        K2 = 2 * k if G == 1 else k + k // G
        f32, i32, i64 = torch.float32, torch.int32, torch.int64
        self.run = torch.zeros(R, dtype=f32, device=dev)
        self.fin_score = torch.zeros(R, dtype=f32, device=dev)
        self.fin_flag = torch.zeros(R, dtype=i32, device=dev)
        self.fin_len = torch.zeros(R, dtype=i32, device=dev)
        self.fin_tok = torch.zeros(R, cache.Smax, dtype=i64, device=dev)
        self.fin_stage = torch.zeros(R, cache.Smax, dtype=i64, device=dev)
        self.hist_stage = torch.zeros(R, cache.Smax, dtype=i64, device=dev)
        self.unsat = torch.ones(self.B * G, dtype=i32, device=dev)
        self.parent = torch.arange(R, dtype=i32, device=dev)
        self.cand_score = torch.zeros(R, K2, dtype=f32, device=dev)
        self.cand_tok = torch.zeros(R, K2, dtype=i32, device=dev)
        self.kstage, self.vstage = torch.empty_like(cache.k), torch.empty_like(cache.v)
        self.bufs = dict(run=self.run, fin_score=self.fin_score, fin_flag=self.fin_flag, fin_len=self.fin_len,
                         fin_tok=self.fin_tok, fin_stage=self.fin_stage, hist=cache.history, hist_stage=self.hist_stage,
                         unsat=self.unsat, parent=self.parent, token=token)

    def reset(self, eos: int):
        """State at the start of a generate() call (enqueued, no sync)."""
        self.run.view(self.B * self.G, self.k // self.G).fill_(-1e9)[:, 0] = 0.0
        self.fin_score.fill_(-1e9)
        self.fin_flag.zero_()
        self.fin_len.zero_()
        self.fin_tok.fill_(eos)
        self.unsat.fill_(1)


class ContrastBuffers:
    """Device state of contrastive search over a KV cache of R = B * k rows (DESIGN.md "Contrastive search"): the context store
    ``ctx`` (B, Smax, d) bf16 of ln_f outputs -- one row per prompt position, then one per generated token --, its valid length per
    sample, the row of every sample's group that was selected last (``src``), the candidates' probabilities and the per-chunk
    partial maxima of the similarity launch.  The candidates' ids live in the decode state's token rows."""

    def __init__(self, cache: KVCache, k: int, d: int):
        R, dev = cache.B, cache.k.device
        assert R % k == 0
        self.k, self.B, self.Tmax = k, R // k, cache.Smax
        self.ctx = torch.zeros(self.B, self.Tmax, d, dtype=BF16, device=dev)
        self.ctx_len = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.src = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.cand_p = torch.zeros(self.B, k, dtype=torch.float32, device=dev)
        self.part = torch.zeros(self.B, ops.contrastive_chunks(self.Tmax), k, dtype=torch.float32, device=dev)


class ConstraintMode:
    """LMEngine.constraint_mode's checked constraint: the host copies of the table and the per-row roots (sampling.trie_forest)
    and the largest token id."""

    def __init__(self, tries):
        from .sampling import trie_forest
        self.table, self.roots = trie_forest(tries)
        self.max_token = max(max(t.tokens()) for t in {id(t): t for t in tries}.values())


class SlotConstraint:
    """The constraint of a slot plan (DESIGN.md "Choosing over a request stream"): every row walks a trie of its own, and the
    SESSION keeps the device table and the roots (engine.SlotSession: the forest of the live slots' tries, rebuilt when an
    admission changes the set) -- the plan only says that the step's launch is the constrained one."""
    table = roots = None


class StepKey(NamedTuple):
    """What the launches of a token step depend on (SelectionPlan.graph_key): two steps share a captured graph exactly when their
    keys are equal.  Launch arguments are in it; the contents of the device tables, rewritten between replays, are not."""
    feed_back: bool
    mode: Any                   # None (greedy), the sampling tuple, the beam tuple, or "noselect" (a teacher-forced position)
    proc: Optional[tuple]       # (repetition_penalty, no_repeat_ngram_size, min_new_tokens, NUMBER of suppress ids)
    stop: Optional[tuple]       # (number of eos ids, number of stop sequences, pad id)
    n_top: Optional[int]        # the log-probability buffers' addresses are launch arguments too (KVCache.alloc_logprobs)
    constrained: bool           # the trie buffers' addresses and capacity are launch arguments (KVCache.alloc_trie)
    guidance: Optional[tuple]   # (scale, cut)
    slots: bool = False         # the bookkeeping launch is the slot session's (window, ring history, frozen finished rows)

    @property
    def beam(self) -> bool:
        return isinstance(self.mode, tuple) and self.mode[:1] == ("beam",)

    @property
    def contrast(self) -> bool:
        return isinstance(self.mode, tuple) and self.mode[:1] == ("contrast",)


class SelectionPlan(NamedTuple):
    """The checked modes of one token step (DESIGN.md "The selection plan"), built once per call by LMEngine.selection_plan --
    the only place that normalises the public keywords and refuses their combinations -- and handed down as it is: forward,
    decode, _arm_first_token, _decode_step and select_token read it, nothing below re-checks it."""
    mode: Any = None                        # None (greedy), sample_mode's tuple, beam_mode's tuple, or contrast_mode's tuple
    proc: Optional[tuple] = None            # proc_mode: (repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress ids)
    stop: Optional[tuple] = None            # stop_mode: (eos ids, stop sequences)
    n_top: Optional[int] = None             # logprob_mode
    cons: Optional[ConstraintMode] = None   # constraint_mode
    guidance: Optional[tuple] = None        # guidance_mode: (scale, cut)
    vocab: Optional[int] = None             # V the token ids were checked against (None: arm() cannot check them)
    select: bool = True                     # False: a teacher-forced position, only the KV write position advances
    keys: tuple = ()                        # graph_key of feed_back False / True, computed once (keyed)
    slots: bool = False                     # a slot session's step (SlotSession): per-row stopping with ops.sample_finish_slots

    @property
    def is_beam(self) -> bool:
        return isinstance(self.mode, tuple) and self.mode[:1] == ("beam",)

    @property
    def is_contrast(self) -> bool:
        return isinstance(self.mode, tuple) and self.mode[:1] == ("contrast",)

    @property
    def is_rows(self) -> bool:
        """Per-request sampling (DESIGN.md "Per-request sampling"): mode ("rows", warp) -- every row's settings and seed come from
        the cache's table (``cache.sample_rows``), not from the mode."""
        return isinstance(self.mode, tuple) and self.mode[:1] == ("rows",)

    @property
    def is_speculate(self) -> bool:
        """Speculative decoding (DESIGN.md "Speculative decoding"): mode ("speculate", T, max_ngram) -- every step runs T rows
        per sequence, the last emitted token and up to T - 1 prompt-lookup drafts, and keeps the prefix the model agrees with.
        Sampled rows: ("speculate", T, max_ngram, ("rows", warp)) -- the selection is the chunk launch over the sequences' records."""
        return isinstance(self.mode, tuple) and self.mode[:1] == ("speculate",)

    @property
    def spec_rows(self) -> Optional[bool]:
        """A speculative plan's selection: None (the argmax of every fed row) or ``warp`` of its ("rows", warp) -- every fed row
        under its SEQUENCE's record (cache.spec[T].sample_rows) at the counter count + t (ops.sample_chunk)."""
        return self.mode[3][1] if self.is_speculate and len(self.mode) > 3 else None

    @property
    def spec_launches(self) -> tuple:
        """The two entry points a speculative step enqueues behind the head: the selection and the bookkeeping."""
        assert self.is_speculate
        return ("mg_argmax_f32" if self.spec_rows is None else "mg_sample_chunk_f32",
                "mg_spec_finish_seq" if self.stop[1] else "mg_spec_finish")     # (stop sequences: under ("rows", warp) only)

    @property
    def beam_groups(self) -> tuple:
        """(num_beam_groups, diversity_penalty) of a beam mode: (1, 0.0) for the five-entry tuple of plain beam search."""
        return tuple(self.mode[5:7]) if len(self.mode) > 5 else (1, 0.0)

    @property
    def rewrites_logits(self) -> bool:
        """Something runs in place on the logits in front of the selection: the first token is then selected from a copy (the
        caller's ``.logits`` stay raw), and a step that also reports log-probabilities works on the second logits buffer."""
        return self.proc is not None or self.cons is not None or self.guidance is not None

    @property
    def second_buffer(self) -> bool:
        return self.n_top is not None and self.rewrites_logits

    def without_selection(self) -> "SelectionPlan":
        """The plan of a teacher-forced position of a multi-token call: nothing selected, nothing processed or recorded (a beam
        mode stays, for arm() to find the cache armed for it; the step's key does not read it)."""
        return SelectionPlan(mode=self.mode if self.is_beam else None, vocab=self.vocab, select=False).keyed()

    def keyed(self) -> "SelectionPlan":
        """The plan with both of its step keys computed: a replayed step looks its graph up without building anything."""
        p, s = self.proc, self.stop
        rest = (self.mode if self.select else "noselect", None if p is None else tuple(p[:3]) + (len(p[3]),),
                None if s is None else (len(s[0]), len(s[1]), s[0][0]), self.n_top, self.cons is not None, self.guidance, self.slots)
        return self._replace(keys=(StepKey(False, *rest), StepKey(True, *rest)))

    def graph_key(self, feed_back: bool) -> StepKey:
        return (self.keys or self.keyed().keys)[bool(feed_back)]

    def rows(self, cache: KVCache) -> int:
        """The rows the selection runs over: all of the cache's, or -- guided -- its first half."""
        if self.guidance is None:
            return cache.B
        if cache.B % 2 or cache.pos_stride != 1:
            raise ValueError(f"guidance needs a ragged cache of 2R rows (prompts, then negative prompts), got {cache.B} rows"
                             f"{'' if cache.pos_stride == 1 else ' with one shared position'}")
        return cache.B // 2

    def arm(self, cache: KVCache, st, first: bool = False):
        """What the step's launches read and the step does not write, in the cache's device buffers -- never touched inside a
        captured step: decode() and _arm_first_token call this before anything is captured or replayed.  Token ids are checked
        against the vocabulary; the suppress ids, the stop table, the trie's table and roots are copied only when they differ
        from what the buffers hold (a table that outgrows its buffer re-allocates it: KVCache.alloc_trie); the log-probability
        buffers and -- when something rewrites the logits too -- the second logits buffer are allocated.  ``first``: the call
        that starts a loop marks every row unfinished; a later step finds the cache armed or refuses."""
        dev, V = cache.k.device, self.vocab if self.vocab is not None else float("inf")
        armed = cache.beam is not None and (cache.beam.k, cache.beam.G) == (self.mode[1], self.beam_groups[0]) if self.is_beam else True
        if not first and not armed:
            raise ValueError("beam decoding needs a cache armed for this num_beams (prefill with eos_token= and beam=)")
        if self.is_contrast and not first:
            cb = cache.contrast
            if cb is None or (cb.k, cb.Tmax) != (self.mode[1], cache.Smax):
                raise ValueError("contrastive decoding needs a cache armed for this top_k (prefill with eos_token= and a contrastive plan)")
        if self.proc is not None:
            ids = self.proc[3]
            if any(t >= V for t in ids):
                raise ValueError(f"suppress_tokens must be token ids in [0, {V}), got {[t for t in ids if t >= V]}")
            if cache.suppress is None:
                cache.suppress = torch.zeros(1024, dtype=torch.int32, device=dev)
            if ids and ids != cache.suppress_ids:
                cache.suppress[: len(ids)].copy_(torch.tensor(ids, dtype=torch.int32), non_blocking=True)
                cache.suppress_ids = ids
        if self.stop is not None:
            eos_ids, seqs = self.stop
            if not first and cache.finish is None:
                raise ValueError("per-row stopping needs a cache armed for it (prefill with eos_token= and stop=)")
            ids = list(eos_ids) + [t for q in seqs for t in q]
            if any(t >= V for t in ids):
                raise ValueError(f"eos ids and stop sequences must be token ids in [0, {V}), got {[t for t in ids if t >= V]}")
            if cache.stop_table is None:
                cache.stop_table = torch.zeros(ops.STOP_TABLE_INTS, dtype=torch.int32, device=dev)
                cache.finish = torch.zeros(cache.B, 2, dtype=torch.int32, device=dev)
            if tuple(self.stop) != cache.stop_held:
                cache.stop_table.copy_(ops.stop_table(eos_ids, seqs), non_blocking=True)
                cache.stop_held = tuple(self.stop)
            if first:       # every row unfinished again
                cache.finish.copy_(torch.tensor([[-1, 0]] * cache.B, dtype=torch.int32), non_blocking=True)
        if self.is_rows and (cache.sample_rows is None or cache.sample_rows.shape[0] != cache.B):
            # one record per row (ops.sample_rows_table), greedy until a call or an admission writes the row's own; the table's
            # address is a launch argument of the captured step, its contents are not
            cache.sample_rows = torch.zeros(cache.B, ops.SAMPLE_ROW_BYTES, dtype=torch.uint8, device=dev)
            cache._drop_graphs(lambda key: isinstance(key.mode, tuple) and key.mode[:1] == ("rows",))
        if self.slots:
            if self.stop is None or not cache.ragged or cache.ring_cols < 1:
                raise ValueError("a slot step needs per-row stopping and a ragged cache with ring_cols set (SlotSession)")
            if cache.ring is None or cache.ring.shape[1] != cache.ring_cols:
                cache.slot_table = torch.zeros(cache.B, 2, dtype=torch.int32, device=dev)
                cache.ring = torch.zeros(cache.B, cache.ring_cols, dtype=torch.int64, device=dev)
                cache._drop_graphs(lambda key: key.slots)
        rows = self.rows(cache)
        cons = self.cons
        if isinstance(cons, SlotConstraint):
            if not self.slots or cache.trie_table is None:
                raise ValueError("a slot plan's constraint needs the session's trie buffers (SlotSession allocates them)")
        elif cons is not None:
            if cons.max_token >= V:
                raise ValueError(f"the constraint holds token ids outside [0, {V})")
            if cons.roots.numel() != rows:
                raise ValueError(f"the constraint has {cons.roots.numel()} rows, the cache {rows}")
            cache.alloc_trie(cons.table.numel())
            held = cache.trie_held
            if not (held is cons or (held is not None and torch.equal(held.table, cons.table) and torch.equal(held.roots, cons.roots))):
                cache.trie_table[: cons.table.numel()].copy_(cons.table, non_blocking=True)
                cache.trie_roots[:rows].copy_(cons.roots, non_blocking=True)
                cache.trie_held = cons
        if self.n_top is not None:
            cache.alloc_logprobs(self.n_top)        # (a slot session's: [slots, max_new] -- it has set cache.lp_cols)
            if self.rewrites_logits and st.logits_proc is None:
                st.logits_proc = torch.empty_like(st.logits)


class TokenSelection:
    """LMEngine's token selection: the normalisers of the public selection keywords and ``selection_plan`` over them, the
    once-per-call arming of a cache and the launches behind the head.  Of the engine it reads ``V``, ``d``, ``eps``, ``lnf_g``,
    ``lnf_b`` and ``device`` and calls ``_ensure_decode_state``; of a KVCache, its buffers and ``_drop_graphs``."""

    @classmethod
    def selection_plan(cls, plan=None, *, sampling=None, beam=None, processors=None, stop=None, logprobs=None, constraint=None,
                       guidance=None, vocab: Optional[int] = None, contrast=None, slots: bool = False,
                       speculate=None) -> SelectionPlan:
        """The SelectionPlan of the public selection keywords (forward's), checked: the one place that calls the normalisers
        below and that refuses what beam search and contrastive search (``contrast`` = (top_k, penalty_alpha)) are not combined
        with.  A plan that is already built comes back as it is, so a loop builds one and passes ``plan=`` on every call.
        ``vocab``: the number of logits V the token ids must lie in.  ``slots``: the step of a slot session (SlotSession; DESIGN.md
        "Request streams"): greedy or sampled selection with per-row stopping, and -- "Choosing over a request stream" -- the logits
        processors, log-probabilities and ``constraint=True``: the rows' own tries, whose table the session keeps (SlotConstraint)."""
        if slots and (stop is None or any(v is not None for v in (beam, guidance, contrast))):
            raise NotImplementedError("a slot session selects greedily or by sampling under per-row stopping: beam and contrastive search "
                                      "and guidance are not combined with it yet")
        if slots and constraint is not None and constraint is not True:
            raise ValueError("a slot plan takes constraint=True: the session keeps the tries of its rows")
        if constraint is True and not slots:
            raise ValueError("constraint=True is a slot plan's: pass one TokenTrie per row")
        if plan is not None:
            if any(v is not None for v in (sampling, beam, processors, stop, logprobs, constraint, guidance, contrast)):
                raise ValueError("pass plan= or the selection keywords it was built from, not both")
            return plan
        for what, given in (("per-row stopping is", stop), ("token log-probabilities are", logprobs),
                            ("a constraint is", constraint), ("guidance is", guidance)):
            if beam is not None and given is not None:
                raise NotImplementedError(f"{what} not combined with beam search")
        # ``contrast`` = (top_k, penalty_alpha): contrastive search (DESIGN.md "Contrastive search").  What it is not combined with
        # yet are follow-ups, not design limits: processors would run in front of its top-k, per-row stopping in its finish launch
        for what, given in (("beam search is", beam), ("logits processors are", processors), ("per-row stopping is", stop),
                            ("token log-probabilities are", logprobs), ("a constraint is", constraint), ("guidance is", guidance)):
            if contrast is not None and given is not None:
                raise NotImplementedError(f"{what} not combined with contrastive search")
        # ``speculate`` = (T, max_ngram): speculative decoding (DESIGN.md "Speculative decoding") -- greedy selection, or
        # ``sampling`` = ("rows", warp): every sequence under its own record, seed-exact -- under per-row stopping by eos ids and stop
        # sequences; everything else would have to be applied per fed row, and is a follow-up
        if speculate is not None:
            rows = sampling is not None and tuple(sampling[:1]) == ("rows",)
            for what, given in (("session-wide sampled selection (pass (\"rows\", warp): the seed-exact rule) is", None if rows else sampling),
                                ("beam search is", beam), ("logits processors are", processors),
                                ("token log-probabilities are", logprobs), ("a constraint is", constraint), ("guidance is", guidance),
                                ("contrastive search is", contrast), ("a slot session is", True if slots else None)):
                if given is not None:
                    raise NotImplementedError(f"{what} not combined with speculative decoding yet")
            if stop is None:
                raise NotImplementedError("speculative decoding stops per row: it needs stop=")
            if tuple(stop.get("stop_seqs", ())) and not rows:
                # the argmax plan keeps the launches it had (mg_argmax_f32, mg_spec_finish); a greedy call with stop sequences runs
                # under ("rows", warp) with greedy records -- the first maximum, as mg_argmax_f32 takes it -- and mg_spec_finish_seq
                raise NotImplementedError('speculative decoding takes stop sequences under the per-row selection mode: pass '
                                          'sampling=("rows", warp); a record with temperature 0 selects greedily')
            mode = cls.speculate_mode(speculate) + ((cls.sample_mode(sampling),) if rows else ())
            return SelectionPlan(mode, stop=cls.stop_mode(stop), vocab=vocab).keyed()
        mode = cls.sample_mode(sampling)
        if isinstance(mode, tuple) and mode[:1] == ("rows",) and any(v is not None for v in (beam, guidance, contrast)):
            raise NotImplementedError("per-row sampler settings are not combined with beam search, contrastive search or guidance")
        if beam is not None:
            mode = cls.beam_mode(beam)
        if contrast is not None:
            if sampling is not None:
                raise ValueError("contrastive search is deterministic: it takes no sampling mode")
            mode = cls.contrast_mode(contrast, vocab)
        return SelectionPlan(mode, cls.proc_mode(processors), cls.stop_mode(stop), cls.logprob_mode(logprobs, vocab),
                             cls.constraint_mode(constraint), cls.guidance_mode(guidance), vocab, slots=bool(slots)).keyed()

    @staticmethod
    def sample_mode(sampling):
        """None (greedy), (temperature, top_k, top_p) -- the reference's filters, ops.sample -- or ("warp", temperature, top_k,
        top_p, min_p) -- transformers' sampler, ops.sample_warp (DESIGN.md "transformers' sampler"): the selection mode, with its
        values normalised so that it can key a captured step.  ("rows", warp) -- ops.sample_rows (DESIGN.md "Per-request
        sampling") -- carries no values: every row's are in the cache's table, so one captured step serves any of them."""
        if sampling is None:
            return None
        if sampling[0] == "rows":
            if len(sampling) != 2:
                raise ValueError(f'the per-row selection mode is ("rows", warp), got {sampling!r}')
            return ("rows", bool(sampling[1]))
        if sampling[0] == "warp":
            if len(sampling) != 5:
                raise ValueError(f'the warp selection mode is ("warp", temperature, top_k, top_p, min_p), got {sampling!r}')
            return ("warp", float(sampling[1]), int(sampling[2]), float(sampling[3]), float(sampling[4]))
        return (float(sampling[0]), int(sampling[1]), float(sampling[2]))

    @staticmethod
    def speculate_mode(speculate):
        """("speculate", T, max_ngram): the token-selection mode (and graph key: both are launch arguments) of speculative greedy
        decoding, from (T, max_ngram) -- T rows per sequence and step, 2 to 8; n-grams of at most max_ngram tokens, 1 to 16."""
        T, n = speculate
        for v, lo, hi, what in ((T, 2, 8, "T (rows per sequence and step)"), (n, 1, 16, "max_ngram")):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"speculative decoding takes {what} in [{lo}, {hi}], got {v!r}")
        return ("speculate", T, n)

    @staticmethod
    def contrast_mode(contrast, vocab: Optional[int] = None):
        """("contrast", top_k, penalty_alpha): the token-selection mode (and graph key: both are launch arguments) of contrastive
        search, from (top_k, penalty_alpha) checked by sampling.check_contrastive_args."""
        from .sampling import check_contrastive_args
        k, alpha = contrast
        k, alpha = check_contrastive_args(alpha, k, vocab)
        return ("contrast", k, alpha)

    @staticmethod
    def proc_mode(processors):
        """None (nothing is enqueued) or (repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress ids), from
        sampling.check_processor_args' keywords."""
        if processors is None:
            return None
        from .sampling import check_processor_args
        d = check_processor_args(**processors)
        return None if d is None else (d["repetition_penalty"], d["no_repeat_ngram_size"], d["min_new_tokens"], d["suppress_tokens"])

    @staticmethod
    def constraint_mode(constraint):
        """None (today's launches), a ConstraintMode from one sampling.TokenTrie per row, or -- True -- a slot plan's SlotConstraint."""
        if constraint is True:
            return SlotConstraint()
        return None if constraint is None else ConstraintMode(list(constraint))

    @staticmethod
    def guidance_mode(guidance):
        """None (today's launches) or (guidance_scale, guidance_min_p) as floats: launch arguments of the captured step."""
        if guidance is None:
            return None
        from .sampling import check_guidance_values
        scale, min_p = guidance
        check_guidance_values(scale, min_p)
        return (float(scale), float(min_p))

    @staticmethod
    def stop_mode(stop):
        """None (the reference's rule: mg_sample_finish) or (eos ids, stop sequences), from sampling.check_stop_args' dict.  The
        pad id is the first eos id."""
        if stop is None:
            return None
        from .sampling import check_stop_args
        d = check_stop_args(list(stop["eos_ids"]), list(stop.get("stop_seqs", ())), True)
        return (d["eos_ids"], d["stop_seqs"])

    @staticmethod
    def logprob_mode(logprobs, vocab: Optional[int] = None):
        """None (nothing is launched or allocated) or n_top, the number of alternatives per token."""
        if logprobs is None:
            return None
        n = logprobs
        if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= ops.LOGPROBS_MAX_TOP or (vocab is not None and n > vocab):
            raise ValueError(f"logprobs must be None or an integer in [0, min({ops.LOGPROBS_MAX_TOP}, V = {vocab})], got {n!r}")
        return n

    def _arm_first_token(self, out: LMOutput, logits, cache: KVCache, eos_token, seed, plan: SelectionPlan):
        """generate(): the first token of the loop selected from the prefill / extend logits, device-side bookkeeping armed.
        Under a per-row plan (plan.is_rows) ``seed`` is the rows' host table (ops.sample_rows_table): it goes into
        cache.sample_rows, and token 0 is selected by the step's own launch at counter 0."""
        if cache.eos != int(eos_token):        # the eos id is a launch argument of the captured bookkeeping kernel
            cache.eos = int(eos_token)
            cache._drop_graphs()
        cache.sample_state.copy_(torch.tensor([0, -1], dtype=torch.int32), non_blocking=True)
        if seed is not None and not plan.is_rows and not plan.is_speculate:
            cache.seed.fill_(int(seed) & 0x7fffffffffffffff)
        if plan.is_speculate:                      # its own decode state (B * T rows), kept apart from the plain step's
            return self._arm_speculate(out, logits, cache, eos_token, seed, plan)
        st = self._ensure_decode_state(cache)      # the first token lands where the decode steps read it back
        if plan.is_beam:
            self._arm_beam(cache, st, plan.mode)
        elif cache.beam is not None:
            # a pooled cache that last served beam search starts a greedy / sampled call: without its beam buffers (the K / V
            # staging copies are as large as the cache) and the steps captured on them -- it may be handed to the caller and
            # continued (extend refuses a cache that is mid-beam)
            cache.beam = None
            cache._drop_graphs(lambda key: key.beam)
        if plan.stop is not None and int(eos_token) != plan.stop[0][0]:
            raise ValueError(f"per-row stopping pads with the first eos id: eos_token must be {plan.stop[0][0]}, got {eos_token}")
        plan.arm(cache, st, first=True)
        if plan.is_rows:
            if not torch.is_tensor(seed) or tuple(seed.shape) != tuple(cache.sample_rows.shape) or seed.dtype != torch.uint8:
                raise ValueError(f"a per-row plan takes the rows' table as seed=: uint8 {tuple(cache.sample_rows.shape)} "
                                 "(ops.sample_rows_table)")
            cache.sample_rows.copy_(seed, non_blocking=True)
        if plan.is_contrast:
            # no token yet: selecting one needs its candidates' hidden states, so the prefill's logits give the first candidate set
            self._arm_contrast(cache, st, plan, logits)
            out["next_token"], out["eos_state"] = None, cache.sample_state
            return
        # step 0 of the rules runs on a copy: the caller's .logits stay raw
        out["next_token"] = self.select_token(logits.clone() if plan.rewrites_logits else logits, cache, plan, out=st.token, raw=logits)
        out["eos_state"] = cache.sample_state

    def _arm_speculate(self, out: LMOutput, logits, cache: KVCache, eos_token, spec, plan: SelectionPlan):
        """generate(), speculative: token 0 selected from the prefill logits and the first drafts made by the arming call of the
        bookkeeping launch (ops.spec_finish, arm=True).  ``spec`` (in place of a seed): dict(limit = max_steps, lookup = None or B
        lists of token ids, rows = a sampled plan's table of the B sequences' records, ops.sample_rows_table).  The cache turns ragged -- the rows advance by different amounts --,
        the state of the T-row step lives in cache.spec[T] (_ensure_spec_state)."""
        T, n = plan.mode[1:3]
        warp, n_seq = plan.spec_rows, len(plan.stop[1]) if plan.stop is not None and plan.stop[1] else None
        if not isinstance(spec, dict) or "limit" not in spec:
            raise ValueError("a speculative plan takes dict(limit=max_steps, lookup=None or one id list per row) as seed=")
        if plan.stop is None or int(eos_token) != plan.stop[0][0]:
            raise ValueError("speculative decoding pads with the first eos id: eos_token must be the plan's first eos id")
        if not cache.ragged:
            cache.set_rows(cache.rows_pos())
        st = self._ensure_spec_state(cache, T)
        if st.refusal is not None:
            raise NotImplementedError(st.refusal)
        limit, B, dev = int(spec["limit"]), cache.B, cache.k.device
        # rows never pass their prompt + limit, and a step writes T positions from there: inside the cache, or refused here (the
        # host mirror cache.pos only bounds the positions from above until the loop ends)
        if limit < 0 or int(cache.rows_pos().max()) + limit + T > cache.Smax:
            raise ValueError(f"KV cache too small (Smax={cache.Smax}) for {limit} tokens of T = {T} rows: pass cache_hint = max_steps + T")
        rows = spec.get("lookup") or [[] for _ in range(B)]
        if len(rows) != B:
            raise ValueError(f"lookup has {len(rows)} rows, the cache {B}")
        if any(not 0 <= int(t) < self.V for q in rows for t in q):
            raise ValueError(f"lookup ids must be token ids in [0, {self.V})")
        longest = max(len(q) for q in rows)
        if longest > st.lookup.shape[1]:             # grown, never shrunk: its address and width are launch arguments
            st.lookup = torch.zeros(B, ops.ceil_to(longest, 256), dtype=torch.int32, device=dev)
            st.graphs.clear()
        if longest:
            host = torch.zeros(B, longest, dtype=torch.int32)
            for b, q in enumerate(rows):
                host[b, :len(q)] = torch.tensor([int(t) for t in q], dtype=torch.int32)
            st.lookup[:, :longest].copy_(host, non_blocking=True)
        st.lookup_len.copy_(torch.tensor([len(q) for q in rows], dtype=torch.int32), non_blocking=True)
        for t in (st.n_draft, st.count, st.stats):
            t.zero_()
        if warp is not None:                         # the sequences' records, written once per call: the captured step reads the table
            table = spec.get("rows")
            if not torch.is_tensor(table) or tuple(table.shape) != tuple(st.sample_rows.shape) or table.dtype != torch.uint8:
                raise ValueError(f"a sampled speculative plan takes the sequences' table as rows=: uint8 {tuple(st.sample_rows.shape)} "
                                 "(ops.sample_rows_table)")
            st.sample_rows.copy_(table, non_blocking=True)
        st.limit, st.armed = limit, True
        plan.arm(cache, st, first=True)
        if warp is None:
            ops.argmax(logits, out=st.token[:B])
        else:       # the chunk selection at T = 1 over the zeroed counts: token 0 of every sequence, drawn at counter 0
            ops.sample_chunk(logits, 1, st.sample_rows, st.count, cache.finish, history_cols=cache.history.shape[1], warp=warp,
                             out=st.token[:B])
        ops.spec_finish(st.ids.view(B, T), st.n_draft, st.token, cache.history, st.count, cache.finish, cache.stop_table,
                        len(plan.stop[0]), limit, st.lookup, st.lookup_len, st.stats, cache.sample_state, T - 1, n, self.V, arm=True,
                        **({} if n_seq is None else dict(n_seq=n_seq)))
        out["next_token"], out["eos_state"] = st.token[:B], cache.sample_state

    @staticmethod
    def beam_mode(beam):
        """("beam", num_beams, length_penalty, early_stopping, max_steps): the token-selection mode (and graph key) of beam search,
        from those four values -- or, followed by (num_beam_groups, diversity_penalty) with more than one group, the seven-entry
        mode of diverse beam search: G and the penalty are launch arguments.  One group gives the five-entry tuple as it was."""
        from .sampling import check_beam_args
        k, lp, es, n = beam[:4]
        G, lam = beam[4:] if len(beam) > 4 else (1, 0.0)
        es = check_beam_args(int(k), 1, es, G, lam)
        mode = ("beam", int(k), float(lp), es, int(n))
        return mode if G == 1 else mode + (int(G), float(lam))

    def _arm_beam(self, cache: KVCache, st, mode):
        """Beam buffers of this cache for num_beams = k (in G groups) of the beam ``mode`` (re-allocated -- and the captured steps
        dropped -- when (k, G) changes), reset for a new generate() call."""
        k, G = mode[1], mode[5] if len(mode) > 5 else 1
        if cache.B % k:
            raise ValueError(f"beam search over {cache.B} cache rows with num_beams = {k}: rows must be samples x num_beams")
        need = 2 * k if G == 1 else k + k // G            # the length of a row's candidate list
        if need > self.V:
            raise ValueError(f"num_beams = {k}{'' if G == 1 else f' in {G} groups'} needs a vocabulary of at least {need} tokens")
        if cache.beam is None or (cache.beam.k, cache.beam.G) != (k, G):
            cache.beam = BeamBuffers(cache, k, st.token, G)
            st.graphs.clear()
        cache.beam.reset(cache.eos)

    def _arm_contrast(self, cache: KVCache, st, plan: SelectionPlan, logits: torch.Tensor):
        """The once-per-call work of contrastive search, outside any capture: the buffers of this cache for top_k = k (re-allocated
        -- and the steps captured on them dropped -- when (k, Smax) changes), the prompt's ln_f outputs into the context store (the
        k rows of a sample hold the same prompt: row b * k is read), ctx_len = the prompt lengths, and the first candidate set from
        the prefill's logits into the token rows the first step embeds."""
        _, k, _ = plan.mode
        R = cache.B
        x, cache.prefill_x = cache.prefill_x, None
        if R % k:
            raise ValueError(f"contrastive search over {R} cache rows with top_k = {k}: rows must be samples x top_k")
        if k > self.V:
            raise ValueError(f"top_k = {k} needs a vocabulary of at least {k} tokens")
        if x is None:
            raise ValueError("contrastive search is armed by the prefill call (inputs_embeds with eos_token= and the plan)")
        cb = cache.contrast
        if cb is None or (cb.k, cb.Tmax) != (k, cache.Smax):
            cache.contrast = cb = ContrastBuffers(cache, k, self.d)
            cache._drop_graphs(lambda key: key.contrast)
        B, S = R // k, x.shape[1]
        h = ops.layernorm(x[::k].reshape(B * S, self.d), self.lnf_g, self.lnf_b, self.eps)     # the op every later hidden row comes from
        cb.ctx[:, :S].copy_(h.view(B, S, self.d))
        cb.ctx_len.copy_(cache.rows_pos()[::k].to(torch.int32), non_blocking=True)
        cb.src.copy_(torch.arange(0, R, k, dtype=torch.int32), non_blocking=True)
        ops.contrastive_topk(logits, cb.src, k, st.token, cb.cand_p)

    def _select_contrast(self, x: torch.Tensor, cache: KVCache, st, plan: SelectionPlan):
        """The contrastive step's launches behind the head (DESIGN.md "Contrastive search"): ln_f of the candidates' rows (the wide
        step has it in st.lnf already), the similarity against the context store, the selection with greedy decoding's
        bookkeeping, the selected row's new K / V to its siblings, the next candidate set from the selected row's logits."""
        cb = cache.contrast
        _, k, alpha = plan.mode
        if cache.B <= 16:
            ops.layernorm(x, self.lnf_g, self.lnf_b, self.eps, out=st.lnf)
        ops.contrastive_sim(st.lnf, cb.ctx, cb.ctx_len, k, cb.part, len_max=cache.pos)
        ops.contrastive_finish(cb.part, cb.cand_p, alpha, st.lnf, cb.ctx, cb.ctx_len, cb.src, st.token, cache.eos, cache.sample_state,
                               cache.pos, d_pos=cache.d_pos, history=cache.history, pos_stride=cache.pos_stride)
        ops.kv_broadcast(cache.k, cache.v, k, cb.src, cache.d_pos, pos_stride=cache.pos_stride, pos_delta=-1)
        ops.contrastive_topk(st.logits[:, : self.V], cb.src, k, st.token, cb.cand_p)

    def _select_beam(self, logits: torch.Tensor, cache: KVCache, plan: SelectionPlan, advance: bool):
        """The beam step's three launches: per-row top 2k, the bookkeeping of every sample, the K / V reorder by parent.  With
        processors, their launch has already turned the rows into (processed) log_softmax scores.  With G > 1 groups the lists
        are k + k / G long (bm.cand_score's width) and the bookkeeping launch is the grouped one; nothing else differs."""
        bm = cache.beam
        _, k, lp, es, max_steps = plan.mode[:5]
        G, lam = plan.beam_groups
        ops.beam_topk(logits, bm.run, bm.cand_score, bm.cand_tok, normalized=plan.proc is not None)
        pos = dict(d_pos=cache.d_pos if advance else None, pos_stride=cache.pos_stride)
        if G == 1:
            ops.beam_finish(bm.cand_score, bm.cand_tok, bm.B, k, logits.shape[1], cache.eos, lp, es, max_steps, cache.sample_state,
                            bm.bufs, **pos)
        else:
            ops.beam_finish_groups(bm.cand_score, bm.cand_tok, bm.B, k, G, lam, logits.shape[1], cache.eos, lp, es, max_steps,
                                   cache.sample_state, bm.bufs, **pos)
        ops.kv_reorder(cache.k, cache.v, bm.kstage, bm.vstage, bm.parent, cache.d_pos, pos_stride=cache.pos_stride)
        return bm.bufs["token"]

    def beam_results(self, cache: KVCache, n_ret: int):
        """(tokens (B*n_ret, n) int64 eos-padded, scores (B*n_ret,) fp32, lengths (B*n_ret,) int64) of the best n_ret finished
        hypotheses per sample (slots are kept in score order); n = the longest of them.  One host sync.  With groups: the
        first n_ret of the sample's slots taken round-robin over the groups by rank within the group (DESIGN.md "Diverse beam
        search")."""
        bm = cache.beam

        def slots(t):       # (B, k, ...) in the order the hypotheses are returned in
            t = t.view(bm.B, bm.G, bm.k // bm.G, *t.shape[1:])
            return (t.transpose(1, 2) if bm.G > 1 else t).reshape(bm.B, bm.k, *t.shape[3:])

        lens = slots(bm.fin_len)[:, :n_ret].reshape(-1).to(torch.int64)
        n = max(1, int(lens.max()))
        toks = slots(bm.fin_tok)[:, :n_ret, :n].reshape(bm.B * n_ret, n)
        return toks.clone(), slots(bm.fin_score)[:, :n_ret].reshape(-1).clone(), lens

    def select_token(self, logits: torch.Tensor, cache: KVCache, plan: SelectionPlan, out: Optional[torch.Tensor] = None,
                     advance: bool = False, raw: Optional[torch.Tensor] = None) -> torch.Tensor:
        """next token of every row from fp32 logits (B, V) under ``plan`` (armed: SelectionPlan.arm): greedy argmax (mode None;
        reference sampling.py:96-97) or the sampled branch (mode = (temperature, top_k, top_p); :99-107 -- or ("warp",
        temperature, top_k, top_p, min_p): transformers' sampler, sample_mode), then the loop bookkeeping in one small launch
        (all-eos step, step counter, token history, and -- inside a decode step -- the KV write position).  Enqueue-only:
        used inside the captured token step and, eagerly, on the prefill logits.  A beam mode (beam_mode) runs the beam step
        instead: the selected token of every row lands in cache.beam's token buffer (the decode state's st.token).
        ``plan.proc`` (the ids already in cache.suppress): the logits processors, one launch IN PLACE on ``logits`` immediately
        before the selection -- on the raw logits, or as log_softmax + rules in front of the beam step.
        ``plan.stop`` (the table already in cache.stop_table): the bookkeeping launch is the per-row one
        (ops.sample_finish_rows) -- a finished row's token becomes the pad id in place --, and min_new_tokens bans every eos id.
        ``plan.n_top`` (the buffers already allocated): one launch AFTER the selection and BEFORE the bookkeeping -- which
        advances the step the launch reads its column from and overwrites a finished row's token -- writes the token's
        log-probability and the n_top alternatives of ``raw`` (default ``logits``): the rows as they were before the processors.
        ``plan.cons`` (table and roots already in the cache's buffers): the processors' launch is the constrained one
        (ops.logits_process_constrained) -- the processors' rules, or neutral values, then the trie constraint with every eos
        id --: with processors as many launches as without a constraint, without them one more.
        ``plan.guidance``: ``logits`` / ``raw`` / ``out`` hold 2R rows.  First ops.logits_guidance in place on rows [0, R) against
        rows [R, 2R); then all of the above over the first R rows of everything; last ops.guidance_follow mirrors the tokens
        into ``out[R:]`` and advances the positions of rows [R, 2R).  Two launches more.  Returns the R tokens."""
        mode, proc, stop, n_top, cons, guidance = plan[:6]
        half = None
        if guidance is not None:
            R = plan.rows(cache)
            assert out is not None and logits.shape[0] == 2 * R and not plan.is_beam
            ops.logits_guidance(logits[:R], logits[R:], guidance[0], guidance[1])
            half, logits, raw, out = out, logits[:R], None if raw is None else raw[:R], out[:R]
        rows = (lambda t: t) if guidance is None else (lambda t: None if t is None else t[:R])   # the per-row buffers' share
        more = {} if stop is None or len(stop[0]) < 2 else dict(eos_more=cache.stop_table[1:ops.STOP_MAX_EOS], n_eos_more=len(stop[0]) - 1)
        # a slot step (plan.slots): the same launches through the slot entry points -- the rows' tokens are windows of the ring
        window = (cache.slot_table, cache.finish) if plan.slots else ()
        if cons is not None:
            rules = proc if proc is not None else (1.0, 0, 0, ())
            launch = ops.logits_process_constrained_slots if plan.slots else ops.logits_process_constrained
            launch(logits, cache.sample_state, cache.ring if plan.slots else rows(cache.history), cache.trie_table, cache.trie_roots,
                   cache.trie_path, *window, repetition_penalty=rules[0], no_repeat_ngram_size=rules[1],
                   min_new_tokens=rules[2], eos=cache.eos, suppress=cache.suppress, n_suppress=len(rules[3]), **more)
        elif proc is not None and plan.slots:
            ops.logits_process_slots(logits, cache.sample_state, cache.ring, *window, repetition_penalty=proc[0],
                                     no_repeat_ngram_size=proc[1], min_new_tokens=proc[2], eos=cache.eos, suppress=cache.suppress,
                                     n_suppress=len(proc[3]), **more)
        elif proc is not None:
            ops.logits_process(logits, cache.sample_state, rows(cache.history), repetition_penalty=proc[0], no_repeat_ngram_size=proc[1],
                               min_new_tokens=proc[2], eos=cache.eos, suppress=cache.suppress, n_suppress=len(proc[3]),
                               normalize=plan.is_beam, **more)
        if plan.is_beam:
            return self._select_beam(logits, cache, plan, advance)
        if mode is None:
            tok = ops.argmax(logits, out=out)
        elif mode[0] == "rows":     # every row under its own record; a slot step: at the occupant's own token index, idle rows skipped
            tok = ops.sample_rows(logits, cache.sample_rows, cache.sample_state, mode[1], out=out,
                                  **(dict(slot=cache.slot_table, finish=cache.finish, history_cols=cache.ring_cols) if plan.slots else {}))
        elif mode[0] == "warp":
            tok = ops.sample_warp(logits, mode[1], mode[2], mode[3], mode[4], cache.seed, cache.sample_state, out=out)
        else:
            tok = ops.sample(logits, mode[0], mode[1], mode[2], cache.seed, cache.sample_state, out=out)
        if n_top is not None and plan.slots:
            ops.token_logprobs_slots(logits if raw is None else raw, tok, cache.lp, cache.top_id if n_top else None,
                                     cache.top_lp if n_top else None, cache.sample_state, *window, cache.ring_cols)
        elif n_top is not None:
            ops.token_logprobs(logits if raw is None else raw, tok, rows(cache.lp), rows(cache.top_id) if n_top else None,
                               rows(cache.top_lp) if n_top else None, state=cache.sample_state)
        if plan.slots:
            assert guidance is None
            ops.sample_finish_slots(tok, cache.sample_state, cache.stop_table, len(stop[0]), len(stop[1]), stop[0][0], cache.finish,
                                    cache.slot_table, cache.ring, d_pos=cache.d_pos if advance else None)
        elif stop is not None:
            ops.sample_finish_rows(tok, cache.sample_state, cache.stop_table, len(stop[0]), len(stop[1]), stop[0][0],
                                   rows(cache.finish), d_pos=cache.d_pos if advance else None, history=rows(cache.history),
                                   pos_stride=cache.pos_stride)
        else:
            ops.sample_finish(tok, cache.eos, cache.sample_state, d_pos=cache.d_pos if advance else None,
                              history=rows(cache.history), pos_stride=cache.pos_stride)
        if half is not None:        # after the bookkeeping: a finished row's pad id is mirrored too
            ops.guidance_follow(half, cache.d_pos if advance else None, R, pos_stride=cache.pos_stride)
        return tok
