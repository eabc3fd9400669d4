"""Recorder of the launches LMEngine enqueues, and the cases tests/golden/decode_launch_trace.json pins.

``record(eng, fn, ...)`` replaces, for the duration of ``fn()``, the ``ops`` entry points the engine calls with wrappers that
write down the call and then make it.  A record names the op and every argument:

  * a weight by the engine attribute that holds it (``L0.mlp_adapter[0]``, ``L1.w8.fc_out``, ``head_dec``), with its class, N, K,
    Kp and bias;
  * a tensor by the buffer it lives in -- a field of the decode state (``st.ctx_t``), of the cache, of the engine, the caller's
    input -- with its column range, rows and row stride; a tensor that lives in none of them (the prefill's locals) by the
    record that last wrote it (``@12``: the value record 12 returned, ``@12.out``: the buffer record 12 was handed as ``out``);
  * scalars (activation codes, ``variant``, ``tile``, ``pos_stride``, eps ...) as they are, arguments left at their default
    omitted.  ``ln_fold`` / ``split`` / ``residuals`` / ``scale`` appear when they are passed.

Exchanging two buffers, two weights or two launches changes the record; values never enter it.  Every tensor a trace sees is kept
alive until the trace ends, so that the allocator cannot hand a freed address to an unrelated tensor.

Run as a script it prints the traces of ``CASES`` as JSON: that output, made on the commit before a change to the token step or
the prefill, is the golden file; tests/test_launch_trace_gpu.py compares the same cases against it.

``SELECT_CASES`` / ``run_select_case`` record the token-selection ops alone (SELECT_OPS: what runs behind the head, for the first
token of a call and for one cached step, under every selection mode); ``python tests/launch_trace.py select`` prints
tests/golden/selection_launch_trace.json, made on the commit before a change to how the modes reach the step.

The last part records a ``MagmaEngine``: what ``_lm_forward`` and ``_lm_backward`` launch in one training step (TrainTrace,
``TRAIN_CASES``, ``run_train_case``), with the bits of the loss and a digest of every gradient.  ``python tests/launch_trace.py train``
prints tests/golden/train_launch_trace.json, which tests/test_train_launch_trace_gpu.py compares against."""
import inspect
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OPS = ("embedding", "layernorm", "gemm", "gemm_skinny", "gemm_skinny2", "decode_attn_gemv", "attn_decode_fused", "gelu_erf",
       "rotary_split", "attn_prefill", "attn_prefill_cached", "quantize_rows_fp8", "quantize_mx_fp8", "gemm_fp8", "gemm_mx_fp8",
       "rotary_split_fp8", "attn_prefill_fp8", "argmax", "sample", "sample_finish", "advance_pos")
# arguments an op writes (paths into the bound arguments); a returned value that is none of them is registered as "@i"
WRITES = {"embedding": ["out"], "layernorm": ["out"], "gemm": ["out", "out2"], "gemm_skinny": ["out", "split.1", "out2"],
          "gemm_skinny2": ["a.2", "a.3.split.1", "b.2", "b.3.split.1"], "decode_attn_gemv": ["attn_out", "gemv.2", "gemv.3.split.1"],
          "attn_decode_fused": ["out"], "gelu_erf": ["out"], "rotary_split": ["q_out", "kcache", "vcache", "vt"],
          "attn_prefill": ["out", "lse"], "attn_prefill_cached": ["out"], "gemm_fp8": ["out"], "gemm_mx_fp8": ["out"],
          "attn_prefill_fp8": ["out", "lse"], "argmax": ["out"], "sample": ["out"]}
GEMV_TUPLES = {"gemm_skinny2": ("a", "b"), "decode_attn_gemv": ("gemv",)}      # (x, w, out, kwargs) descriptors


def _span(t):
    """Bytes from t's first element to one past its last."""
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size() if t.numel() else 0


def _is_weight(o):
    return hasattr(o, "N") and hasattr(o, "K") and (hasattr(o, "ft") or hasattr(o, "rm"))


class Trace:
    def __init__(self, eng, cache=None, inputs=None):
        self.eng, self.cache, self.inputs = eng, cache, dict(inputs or {})
        self.records = []
        self._written = []        # (start, end, name, row stride of the written tensor), in write order
        self._objects = {}        # id(returned non-tensor object) -> name
        self._keep = []
        self.on = True
        self.writes = WRITES
        self.rename = {}          # argument name -> key in the record

    # ---- names -------------------------------------------------------------------------------------------------------------
    def _walk(self, name, o, tensors, weights, depth=0):
        from magma_amd import engine
        if torch.is_tensor(o):
            tensors.append((name, o))
        elif _is_weight(o):
            weights.append((name, o))
            for k, v in sorted(vars(o).items()):
                if torch.is_tensor(v) or (_is_weight(v) and v is not o and depth < 4):   # (a _par_up copy holds itself)
                    self._walk(f"{name}.{k}", v, tensors, weights, depth + 1)
        elif isinstance(o, (tuple, list)):
            for i, v in enumerate(o):
                self._walk(f"{name}[{i}]", v, tensors, weights, depth + 1)
        elif isinstance(o, dict):
            for k, v in o.items():
                self._walk(f"{name}[{k!r}]", v, tensors, weights, depth + 1)
        elif isinstance(o, engine._Layer) and depth < 4:
            for k, v in sorted(vars(o).items()):
                if k != "_src":
                    self._walk(f"{name}.{k}" if name else k, v, tensors, weights, depth + 1)

    def _names(self):
        """(named tensors, named weights) of the engine, the cache and its decode state, the caller's inputs -- walked anew for
        every record: operands are built lazily."""
        tensors, weights = [], []
        for k, v in sorted(vars(self.eng).items()):
            if k == "layers":
                for i, ly in enumerate(v):
                    self._walk(f"L{i}", ly, tensors, weights)
            elif torch.is_tensor(v) or _is_weight(v):
                self._walk(k, v, tensors, weights)
        cache = self.cache
        if cache is None and len(self.eng._cache_pool) == 1:
            cache = next(iter(self.eng._cache_pool.values()))
        if cache is not None:
            for k in ("k", "v", "d_pos", "sample_state", "seed", "history"):
                tensors.append((f"cache.{k}", getattr(cache, k)))
            if cache.decode_state is not None:
                self._walk("st", cache.decode_state, tensors, weights)
        tensors += list(self.inputs.items())
        return tensors, weights

    def _tensor(self, t, tensors):
        p = t.data_ptr()
        best = None
        for name, b in tensors:
            if b.device == t.device and b.data_ptr() <= p < b.data_ptr() + max(_span(b), 1):
                key = (_span(b), name)
                if best is None or key < best[0]:
                    best = (key, name, b.data_ptr(), b.stride(0) if b.ndim == 2 else 0)
        if best is None:
            for start, end, name, ld in reversed(self._written):
                if start <= p < end:
                    best = (None, name, start, ld)
                    break
        if best is None:
            buf, off, ld = "?", 0, 0
        else:
            buf, off, ld = best[1], (p - best[2]) // t.element_size(), best[3]
        dt = str(t.dtype).replace("torch.", "")
        if t.ndim == 2 and t.stride(1) == 1:
            ld = ld or t.stride(0)
            r0, c0 = (off // ld, off % ld) if ld else (0, off)
            return f"{buf}[{r0}:{r0 + t.shape[0]}, {c0}:{c0 + t.shape[1]}] ld={t.stride(0)} {dt}"
        return f"{buf}+{off} shape={list(t.shape)} strides={list(t.stride())} {dt}"

    def _describe(self, v, names):
        tensors, weights = names
        if torch.is_tensor(v):
            self._keep.append(v)
            return self._tensor(v, tensors)
        if _is_weight(v):
            name = next((n for n, w in weights if w is v), None)
            if name is None:
                st = v.ft if getattr(v, "ft", None) is not None else v.rm
                same = sorted(n for n, w in weights if (w.N, w.K) == (v.N, v.K) and
                              (w.ft if getattr(w, "ft", None) is not None else w.rm).data_ptr() == st.data_ptr())
                name = same[0] + "~" if same else "?"
            bias = getattr(v, "bias", None)
            return {"w": name, "cls": type(v).__name__, "N": v.N, "K": v.K, "Kp": v.Kp,
                    "bias": None if bias is None else self._tensor(bias, tensors)}
        if isinstance(v, (tuple, list)):
            return [self._describe(x, names) for x in v]
        if isinstance(v, dict):
            return {str(k): self._describe(x, names) for k, x in v.items()}
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return self._objects.get(id(v), type(v).__name__)

    # ---- recording ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _bind(fn, args, kwargs):
        """Arguments by name, those left at (or passed as) their default omitted; **kw of the GEMV entry points folded in."""
        from magma_amd import ops
        sig = inspect.signature(fn)
        if any(p.kind == p.VAR_KEYWORD for p in sig.parameters.values()):
            sig = inspect.signature(ops.skinny_desc)
        ba = sig.bind(*args, **kwargs)
        out = {}
        for k, v in ba.arguments.items():
            d = sig.parameters[k].default
            if d is inspect.Parameter.empty or not (v is d or (not torch.is_tensor(v) and type(v) is type(d) and v == d)):
                out[k] = v
        return out

    @staticmethod
    def _at(bound, path):
        v = bound
        for k in path.split("."):
            if isinstance(v, dict):
                v = v.get(k)
            elif isinstance(v, (tuple, list)) and k.isdigit() and int(k) < len(v):
                v = v[int(k)]
            else:
                return None
        return v

    def call(self, name, fn, args, kwargs):
        from magma_amd import ops
        bound = self._bind(fn, args, kwargs)
        for k in GEMV_TUPLES.get(name, ()):
            x, w, out, kw = bound[k]
            bound[k] = (x, w, out, self._bind(ops.skinny_desc, (x, w, out), kw))
        names = self._names()
        idx = len(self.records)
        rec = {"op": name}
        for k, v in bound.items():
            if k in GEMV_TUPLES.get(name, ()):
                rec[k] = {"x": self._describe(v[0], names), "w": self._describe(v[1], names), "out": self._describe(v[2], names),
                          **{kk: self._describe(vv, names) for kk, vv in v[3].items() if kk not in ("x", "w", "out")}}
            else:
                rec[self.rename.get(k, k)] = self._describe(v, names)
        self.records.append(rec)
        ret = fn(*args, **kwargs)
        written = set()
        for path in self.writes.get(name, ()):
            t = self._at(bound, path)
            if torch.is_tensor(t):
                self._written.append((t.data_ptr(), t.data_ptr() + _span(t), f"@{idx}.{path}", t.stride(0) if t.ndim >= 2 else 0))
                written.add(t.data_ptr())
        rets = ret if isinstance(ret, (tuple, list)) else (ret,)
        for j, r in enumerate(rets):
            nm = f"@{idx}" if len(rets) == 1 else f"@{idx}.{j}"
            if torch.is_tensor(r):
                self._keep.append(r)
                if r.data_ptr() not in written and self._tensor(r, names[0]).startswith("?"):
                    self._written.append((r.data_ptr(), r.data_ptr() + _span(r), nm, r.stride(0) if r.ndim >= 2 else 0))
            elif r is not None and not isinstance(r, (bool, int, float, str)):
                self._keep.append(r)
                self._objects[id(r)] = nm
        return ret


def record(eng, fn, cache=None, inputs=None, trace=None, op_names=OPS):
    """Run fn() with the engine's ops recorded.  Returns (records, fn's result or the exception it raised).  ``trace``: a Trace
    to record into instead of a new one (a TrainTrace records only while its ``on`` is set); ``op_names``: the ops replaced."""
    from magma_amd import ops
    tr = Trace(eng, cache, inputs) if trace is None else trace
    saved = {n: getattr(ops, n) for n in op_names}

    def wrap(n, f):
        return lambda *a, **k: tr.call(n, f, a, k) if tr.on else f(*a, **k)
    for n, f in saved.items():
        setattr(ops, n, wrap(n, f))
    try:
        try:
            res = fn()
        except Exception as e:  # noqa: BLE001
            res = e
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
    return tr.records, res


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _ad(**kw):
    return dict(adapter_type="normal", downsample_factor=4, **kw)


# id -> (environment set before construction, build_reduced_magma arguments, engine attributes, batch, which traces are kept)
CASES = {
    "fold2": ({}, dict(mlp_factor=4), {}, 2, ("prefill", "decode")),
    "fold1": ({"MAGMA_DECODE_FOLD": "1"}, dict(mlp_factor=4), {}, 2, ("decode",)),
    "fold0_grouped": ({"MAGMA_DECODE_FOLD": "0"}, dict(mlp_factor=4), {}, 2, ("decode",)),
    "ungrouped": ({"MAGMA_DECODE_GROUPED": "0"}, dict(mlp_factor=4), {}, 2, ("decode",)),
    "v2": ({}, dict(mlp_factor=4, attn_factor=4), {}, 2, ("prefill", "decode")),
    "v2_r192": ({}, dict(mlp_factor=4, attn_factor=8), {}, 2, ("decode",)),
    "no_adapters": ({}, dict(mlp_factor=None, adapter_config=None), {}, 2, ("decode",)),
    "attn_normal": ({}, dict(mlp_factor=None, attn_factor=8), {}, 2, ("decode",)),
    "parallel": ({}, dict(adapter_config={"mlp": dict(adapter_type="parallel", downsample_factor=4),
                                          "attention": dict(adapter_type="scaled_parallel", downsample_factor=8)}), {}, 2,
                 ("prefill", "decode")),
    "ln_gelu_erf": ({}, dict(adapter_config={"mlp": _ad(add_layernorm=True, activation=torch.nn.GELU)}), {}, 2, ("decode",)),
    "wide_b24": ({}, dict(mlp_factor=4), {}, 24, ("decode",)),
    "w8_grouped": ({}, dict(n_head=4, mlp_factor=1), {"decode_w8": True}, 2, ("decode",)),
    "v2_fp8_all": ({}, dict(mlp_factor=4, attn_factor=4), {"fp8_mode": "all", "fp8_scaling": "row"}, 2, ("prefill",)),
    "chunked": ({}, dict(mlp_factor=4), {}, 2, ("extend",)),
}
REFUSAL = ({}, dict(n_head=4, mlp_factor=4), {"decode_w8": True}, 2, ("decode",))
_ENV = ("MAGMA_DECODE_FOLD", "MAGMA_DECODE_GROUPED")


def run_case(dev, case):
    """{"prefill" | "decode" | "extend": records} of one case (5 prompt rows, one token step), and what decode() returned or raised."""
    from magma_amd.testing import build_reduced_magma
    env, build, attrs, B, keep = case
    saved = {k: os.environ.pop(k, None) for k in _ENV}
    os.environ.update(env)
    try:
        torch.manual_seed(7)
        model = build_reduced_magma(dev, **build)
        model.eval()
        eng = model.lm.engine
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    for k, v in attrs.items():
        setattr(eng, k, v)
    g = torch.Generator().manual_seed(3)
    emb = torch.randn(B, 5, eng.d, generator=g).to(torch.bfloat16).to(dev)
    ids = torch.randint(0, 1000, (B, 1), generator=g).to(dev)
    out = {}
    with torch.no_grad():
        recs, res = record(eng, lambda: eng.prefill(emb, 8, reuse_cache=True), inputs={"embeds": emb})
        if isinstance(res, Exception):
            raise res
        cache = res[1]
        if "prefill" in keep:
            out["prefill"] = recs
        if "extend" in keep:
            more = torch.randn(B, 3, eng.d, generator=g).to(torch.bfloat16).to(dev)
            recs, res = record(eng, lambda: eng.extend(cache, more), cache=cache, inputs={"embeds": more})
            if isinstance(res, Exception):
                raise res
            out["extend"] = recs
        if "decode" in keep:
            recs, res = record(eng, lambda: eng.decode(ids, cache), cache=cache, inputs={"ids": ids})
            out["decode"] = recs
    return out, res


# ---- token selection: what the first token of a call and one cached step launch behind the head -------------------------------------
SELECT_OPS = ("logits_guidance", "logits_process", "logits_process_constrained", "argmax", "sample", "sample_warp", "token_logprobs",
              "sample_finish", "sample_finish_rows", "guidance_follow", "beam_topk", "beam_finish", "kv_reorder", "advance_pos")
SELECT_WRITES = {"logits_guidance": ["cond"], "logits_process": ["logits"], "logits_process_constrained": ["logits"],
                 "argmax": ["out"], "sample": ["out"], "sample_warp": ["out"]}
# the cache's buffers of the selection modes (allocated on first use) and of beam search
_CACHE_SELECT = ("suppress", "stop_table", "finish", "lp", "top_id", "top_lp", "trie_table", "trie_roots", "trie_path")
_BEAM_BUFFERS = ("run", "fin_score", "fin_flag", "fin_len", "fin_tok", "fin_stage", "hist_stage", "unsat", "parent", "cand_score",
                 "cand_tok", "kstage", "vstage")


class SelectTrace(Trace):
    """Trace of the selection ops alone: the cache's selection and beam buffers are named too, and a tensor that lives in no
    named buffer (the prefill's logits, the copy the first token's processors work on) is numbered by first appearance."""

    def __init__(self, eng, cache=None, inputs=None):
        super().__init__(eng, cache, inputs)
        self.writes = SELECT_WRITES
        self._anon = 0

    def _names(self):
        tensors, weights = super()._names()
        cache = self.cache
        if cache is None and len(self.eng._cache_pool) == 1:
            cache = next(iter(self.eng._cache_pool.values()))
        if cache is not None:
            tensors += [(f"cache.{k}", getattr(cache, k)) for k in _CACHE_SELECT if getattr(cache, k) is not None]
            if cache.beam is not None:
                tensors += [(f"cache.beam.{k}", getattr(cache.beam, k)) for k in _BEAM_BUFFERS]
        return tensors, weights

    def _describe(self, v, names):
        if torch.is_tensor(v) and self._tensor(v, names[0])[:2] in ("?+", "?["):      # in no buffer, not numbered yet
            self._written.append((v.data_ptr(), v.data_ptr() + _span(v), f"?{self._anon}", v.stride(0) if v.ndim >= 2 else 0))
            self._anon += 1
        return super()._describe(v, names)


_PROC =dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=1, suppress_tokens=[11, 12])
_PROC_CONS = dict(_PROC, no_repeat_ngram_size=0)       # (a constraint refuses the n-gram rule)
_STOP = dict(eos_ids=[0, 7], stop_seqs=[[21, 22]])
_STOP2 = dict(eos_ids=[0, 7])
_GUIDE = (1.5, 0.05)
_BEAM = (2, 1.0, False, 8)
# id -> (keywords of the first-token call and of the cached step, "guided" | "beam" | "two_tokens" | "extend" | None).
# ``constraint: True`` stands for one TokenTrie per selecting row.
SELECT_CASES = {
    "greedy": ({}, None),
    "sample": (dict(sampling=(0.7, 5, 0.9)), None),
    "warp": (dict(sampling=("warp", 0.7, 5, 0.9, 0.05)), None),
    "processors": (dict(processors=_PROC), None),
    "stop": (dict(stop=_STOP), None),
    "logprobs0": (dict(logprobs=0), None),
    "logprobs3": (dict(logprobs=3), None),
    "processors_logprobs": (dict(processors=_PROC, logprobs=3), None),
    "constraint": (dict(constraint=True), None),
    "constraint_all": (dict(constraint=True, processors=_PROC_CONS, stop=_STOP2, logprobs=3), None),
    "guidance": (dict(guidance=_GUIDE), "guided"),
    "guidance_logprobs": (dict(guidance=_GUIDE, logprobs=3), "guided"),
    "guidance_all": (dict(guidance=_GUIDE, constraint=True, processors=_PROC_CONS, stop=_STOP2, logprobs=3,
                          sampling=(0.7, 5, 0.9)), "guided"),
    "beam": (dict(beam=_BEAM), "beam"),
    "beam_processors": (dict(beam=_BEAM, processors=_PROC), "beam"),
    "two_tokens": (dict(sampling=(0.7, 5, 0.9), processors=_PROC), "two_tokens"),
    "extend": (dict(processors=_PROC, stop=_STOP), "extend"),
}


def run_select_case(dev, case):
    """{"first": the selection launches of the first token (forward(..., eos_token=, seed=) on the prefill logits -- "extend": on
    the logits of inputs_embeds appended to a cache), "step": those of one cached step, eager, the selected tokens fed back --
    "two_tokens": of one call with two input ids per row}: the reduced model, 2 selecting rows, 5 prompt positions."""
    from magma_amd.sampling import TokenTrie
    from magma_amd.testing import build_reduced_magma
    kw, kind = case
    torch.manual_seed(7)
    model = build_reduced_magma(dev, mlp_factor=4)
    model.eval()
    eng = model.lm.engine
    R = 2
    B = 2 * R if kind in ("guided", "beam") else R
    if kw.get("constraint") is True:
        kw = dict(kw, constraint=[TokenTrie([[31, 32], [31, 33, 34]]), TokenTrie([[41], [42, 43]])])
    g = torch.Generator().manual_seed(3)
    emb = torch.randn(B, 5, eng.d, generator=g).to(torch.bfloat16).to(dev)
    first = dict(kw, eos_token=0, seed=5)
    if kind == "guided":
        first["lengths"] = torch.tensor([5, 4, 3, 5])
    out = {}
    with torch.no_grad():
        if kind == "extend":
            cache = eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=16).past_key_values
            more = torch.randn(B, 3, eng.d, generator=g).to(torch.bfloat16).to(dev)
            call = lambda: eng.forward(inputs_embeds=more, use_cache=True, past_key_values=cache, cache_hint=8, **first)  # noqa: E731
        else:
            cache = None
            call = lambda: eng.forward(inputs_embeds=emb, use_cache=True, cache_hint=8, reuse_cache=True, **first)  # noqa: E731
        tr = SelectTrace(eng, cache)
        out["first"], res = record(eng, call, trace=tr, op_names=SELECT_OPS)
        if isinstance(res, Exception):
            raise res
        cache = res.past_key_values
        tr = SelectTrace(eng, cache)
        if kind == "two_tokens":
            ids = torch.randint(0, 1000, (B, 2), generator=g).to(dev)
            eager = eng.decode
            eng.decode = lambda *a, **k: eager(*a, use_graph=False, **k)        # forward() would capture its second step
            try:
                out["step"], res = record(eng, lambda: eng.forward(input_ids=ids, use_cache=True, past_key_values=cache, **kw),
                                          trace=tr, op_names=SELECT_OPS)
            finally:
                del eng.decode
        else:
            out["step"], res = record(eng, lambda: eng.decode(None, cache, use_graph=False, **kw), trace=tr, op_names=SELECT_OPS)
        if isinstance(res, Exception):
            raise res
    return out


# ---- the training step: what MagmaEngine._lm_forward / _lm_backward launch -----------------------------------------------------------
TRAIN_OPS = OPS + ("rotary_qk_inplace", "attn_fwd_rows", "attn_bwd_rows", "transpose", "transpose_colsum", "colsum", "layernorm_bwd",
                   "cross_entropy_fwd_bwd", "gelu_erf_grad_mul", "scale_rows_acc", "mx_empty")
TRAIN_WRITES = {**WRITES, "rotary_qk_inplace": ["qkv"], "rotary_split_fp8": ["qkv"], "attn_fwd_rows": ["out", "lse"],
                "attn_prefill_fp8": ["out", "lse", "mx_out.0", "mx_out.1"], "attn_bwd_rows": ["mx_out.0", "mx_out.1"],
                "transpose": ["out"], "transpose_colsum": ["colsum_out"], "colsum": ["out"], "gelu_erf_grad_mul": ["out"],
                "scale_rows_acc": ["dst"], "gemm_fp8": ["out", "out2", "mx_out.0", "mx_out.1"],
                "gemm_mx_fp8": ["out", "out2", "mx_out.0", "mx_out.1"]}


class TrainTrace(Trace):
    """Trace of a MagmaEngine: records while ``on`` (set inside _lm_forward / _lm_backward, so the image prefix and the trunk
    stay out).  Names: a parameter by its named_parameters() name; the flat optimizer buffers ``g<i>.master`` / ``.grad`` /
    ``.model`` with an element range; the engine's operands (``_out_up[li]``, ``_lm_train_packs``, ``_fp8_packs[key]``,
    ``_ad8_cache[li]``); the LMEngine's layers as the decode traces name them; a RawWeight built for one call by the tensor it
    wraps; an AttnRows by the buffer its rows lie in; everything else by the record that wrote it."""

    def __init__(self, teng, inputs=None):
        super().__init__(teng.module.lm.engine, None, inputs)
        self.teng, self.on, self.writes = teng, False, TRAIN_WRITES
        self.rename = {"op": "operands"}       # attn_prefill_fp8(op=...) must not take the record's "op"
        self._anon = 0

    def _names(self):
        tensors, weights = [], []
        te = self.teng
        for n, p in te.module.named_parameters():
            tensors.append((n, p.data))
        for gi, g in enumerate(te.groups):
            for k in ("master", "grad", "model"):
                tensors.append((f"g{gi}.{k}", getattr(g, k)))
        for k in ("_out_up", "_lm_train_packs", "_fp8_packs", "_ad8_cache"):
            self._walk(k, getattr(te, k), tensors, weights)
        for k, v in sorted(vars(self.eng).items()):
            if k == "layers":
                for i, ly in enumerate(v):
                    self._walk(f"L{i}", ly, tensors, weights)
            elif torch.is_tensor(v) or _is_weight(v):
                self._walk(k, v, tensors, weights)
        tensors += list(self.inputs.items())
        return tensors, weights

    def _describe(self, v, names):
        from magma_amd import ops
        if torch.is_tensor(v) and self._tensor(v, names[0]).startswith("?"):
            # made by torch (an index_select, a zeros, an empty handed over as ``out``): numbered by first appearance
            self._written.append((v.data_ptr(), v.data_ptr() + _span(v), f"?{self._anon}", v.stride(0) if v.ndim >= 2 else 0))
            self._anon += 1
        if isinstance(v, ops.AttnRows):
            return {"rows": [self._describe(t, names) for t in v.keep], "k": (v.k - v.q) // 2, "v": (v.v - v.q) // 2,
                    "ld_row": v.ld_row, "stride_b": v.stride_b, "stride_h": v.stride_h, "B": v.B, "H": v.H, "S": v.S}
        if _is_weight(v) and not any(w is v for _, w in names[1]):
            st = v.ft if getattr(v, "ft", None) is not None else v.rm
            bias = getattr(v, "bias", None)
            return {"w": self._describe(st, names), "cls": type(v).__name__, "N": v.N, "K": v.K, "Kp": v.Kp,
                    "bias": self._describe(bias, names)}
        return super()._describe(v, names)


def _par(mlp_type, attn_type):
    return {"mlp": dict(adapter_type=mlp_type, downsample_factor=4), "attention": dict(adapter_type=attn_type, downsample_factor=8)}


_FP8 = dict(fp8=True, fp8_attn=True, fp8_mx=True, fp8_adapters=True)
# id -> (build_reduced_magma arguments, engine switches (the rest at TRAIN_SWITCHES), "allrows" | "lm_trainable" | None)
TRAIN_CASES = {
    "v1": (dict(mlp_factor=4), {}, None),
    "v1_nocat": (dict(mlp_factor=4), dict(cat_up=False), None),
    "v1_allrows": (dict(mlp_factor=4), {}, "allrows"),
    "v1_recompute": (dict(mlp_factor=4), dict(recompute=True), None),
    "v2": (dict(mlp_factor=8, attn_factor=8), {}, None),
    "attn_only": (dict(mlp_factor=None, attn_factor=8), {}, None),
    "no_adapters": (dict(mlp_factor=None, adapter_config=None), {}, None),
    "parallel": (dict(adapter_config=_par("parallel", "scaled_parallel")), {}, None),
    "ln_gelu_erf": (dict(adapter_config={"mlp": _ad(add_layernorm=True, activation=torch.nn.GELU)}), {}, None),
    "lm_trainable": (dict(mlp_factor=4), {}, "lm_trainable"),
    "fp8_row": (dict(mlp_factor=4), dict(fp8=True, fp8_attn=False, fp8_mx=False), None),
    "fp8_mx": (dict(mlp_factor=4), dict(_FP8, fp8_adapters=False), None),
    "fp8_all": (dict(mlp_factor=2), _FP8, None),
}
TRAIN_SWITCHES = dict(fp8=False, fp8_attn=True, fp8_mx=True, fp8_adapters=True, cat_up=True, recompute=False, truncate=False)


def build_train_case(dev, case):
    """(MagmaEngine in training mode, images, captions, dropout mask) of one case: the reduced two-block model (d = 512,
    d_ff = 2048), B = 2, 64 x 64 images (P = 4), captions of 23 and 11 tokens, data seeds of tests/test_train_gpu.py."""
    from magma_amd.testing import build_reduced_magma
    from magma_amd.train_engine import MagmaEngine
    build, switches, extra = case
    torch.manual_seed(7)
    model = build_reduced_magma(dev, n_layer=2, n_positions=128, **build)
    if extra == "lm_trainable":
        model.config.freeze_lm = False
        for p in model.lm.parameters():
            p.requires_grad = True
    model.config.gradient_accumulation_steps = 1
    eng = MagmaEngine(model)
    eng.train()
    for k, v in {**TRAIN_SWITCHES, **switches}.items():
        setattr(eng, k, v)
    g = torch.Generator().manual_seed(3)
    B, S, P = 2, model.seq_len, 4
    images = torch.randn(B, 3, 64, 64, generator=g)
    caps = torch.full((B, S), model.eos_token, dtype=torch.int64)
    caps[0, :23] = torch.randint(0, 1000, (23,), generator=g)
    caps[1, :11] = torch.randint(0, 1000, (11,), generator=g)
    mask = (torch.rand(B, P, model.lm.engine.d, generator=g) < 0.9).float() / 0.9
    return eng, images.to(dev), caps.to(dev), mask.to(dev)


def run_train_case(dev, case):
    """One forward and one backward of a case.  {"records": the launches inside _lm_forward and _lm_backward, "loss": hex of
    the loss's fp32 bits, "grads": {parameter name: SHA-256 of its fp32 gradient}, "kinds": per block the ``sv["kind"]`` the
    backward read (as lists; None for an engine without _block_backward)} and the engine."""
    import hashlib
    import struct
    from magma_amd import train_engine
    eng, images, caps, mask = build_train_case(dev, case)
    tr = TrainTrace(eng)
    kinds = {}

    def scoped(fn):
        def inner(*a, **k):
            if len(a) == 3:       # _lm_forward(emb, labels, tape)
                tr.inputs.update(emb=a[0], labels=a[1], rows=a[2]["rows"], tgt=a[2]["tgt"])
            tr.on = True
            try:
                return fn(*a, **k)
            finally:
                tr.on = False
        return inner
    eng._lm_forward, eng._lm_backward = scoped(eng._lm_forward), scoped(eng._lm_backward)
    if hasattr(eng, "_block_backward"):
        inner_bb = eng._block_backward

        def block_backward(li, g, sv, tape):
            kinds[li] = list(sv["kind"])
            return inner_bb(li, g, sv, tape)
        eng._block_backward = block_backward
    saved_bottom = train_engine._BOTTOM_PREFIX_ONLY
    train_engine._BOTTOM_PREFIX_ONLY = case[2] != "allrows"
    try:
        def step():
            out = eng(images, caps, dropout_mask=mask)
            eng.backward(out.loss)
            return out.loss
        recs, res = record(eng.module.lm.engine, step, trace=tr, op_names=TRAIN_OPS)
    finally:
        train_engine._BOTTOM_PREFIX_ONLY = saved_bottom
    if isinstance(res, Exception):
        raise res
    name_of = {id(p): n for n, p in eng.module.named_parameters()}
    grads = {name_of[id(p)]: hashlib.sha256(eng.grad_of(p).float().cpu().contiguous().numpy().tobytes()).hexdigest()
             for grp in eng.groups for p in grp.params}
    loss = struct.pack(">f", float(res.float())).hex()
    return {"records": json.loads(json.dumps(recs)), "loss": loss, "grads": grads,
            "kinds": [kinds[li] for li in sorted(kinds)] or None}, eng


def main_train(dev, runs=6):
    """The golden of tests/test_train_launch_trace_gpu.py, one record per line.  Every case runs ``runs`` times: the records and
    the loss must repeat.  A gradient digest is kept only for the tensors whose digest repeated in every run of every case;
    the header's ``unstable`` lists the others (sums formed with fp32 atomics)."""
    w = sys.stdout.write
    results, unstable = {}, set()
    for name, case in TRAIN_CASES.items():
        outs = [run_train_case(dev, case)[0] for _ in range(runs)]
        results[name] = first = outs[0]
        for o in outs[1:]:
            assert o["records"] == first["records"] and o["loss"] == first["loss"], f"{name}: the trace does not repeat"
        unstable |= {n for n, h in first["grads"].items() if any(o["grads"][n] != h for o in outs)}
    w(f'{{"header": {{"runs": {runs}, "unstable": {json.dumps(sorted(unstable))}}},\n "cases": {{\n')
    for ci, (name, first) in enumerate(results.items()):
        stable = {n: h for n, h in first["grads"].items() if n not in unstable}
        w(f' {json.dumps(name)}: {{"loss": {json.dumps(first["loss"])},\n')
        w(f'  "grads": {json.dumps(stable, sort_keys=True)},\n  "records": [\n')
        w(",\n".join("   " + json.dumps(r, sort_keys=True, separators=(",", ":")) for r in first["records"]))
        w("\n  ]}" + ("," if ci + 1 < len(TRAIN_CASES) else "") + "\n")
    torch.cuda.synchronize()
    w("}}\n")


def main():
    dev = torch.device("cuda:0")
    if sys.argv[1:] == ["train"]:
        return main_train(dev)
    if sys.argv[1:] == ["select"]:
        traces = {name: run_select_case(dev, case) for name, case in SELECT_CASES.items()}
        torch.cuda.synchronize()
        sys.stdout.write("{\n" + ",\n".join(
            f' {json.dumps(name)}: {{' + ", ".join(
                f'"{ph}": [\n' + ",\n".join("   " + json.dumps(r, sort_keys=True, separators=(",", ":")) for r in recs) + "\n  ]"
                for ph, recs in sorted(out.items())) + "}" for name, out in traces.items()) + "\n}\n")
        return
    traces = {}
    for name, case in CASES.items():
        out, res = run_case(dev, case)
        if isinstance(res, Exception):
            raise res
        traces[name] = out
    torch.cuda.synchronize()
    json.dump(traces, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
