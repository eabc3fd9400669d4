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
the prefill, is the golden file; tests/test_launch_trace_gpu.py compares the same cases against it."""
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
                rec[k] = self._describe(v, names)
        self.records.append(rec)
        ret = fn(*args, **kwargs)
        written = set()
        for path in WRITES.get(name, ()):
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


def record(eng, fn, cache=None, inputs=None):
    """Run fn() with the engine's ops recorded.  Returns (records, fn's result or the exception it raised)."""
    from magma_amd import ops
    tr = Trace(eng, cache, inputs)
    saved = {n: getattr(ops, n) for n in OPS}

    def wrap(n, f):
        return lambda *a, **k: tr.call(n, f, a, k)
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


def main():
    dev = torch.device("cuda:0")
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
