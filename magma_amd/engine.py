"""LMEngine -- executes the GPT-J(+adapters) graph on the HIP kernels.

One engine per GPTJForCausalLM.  It owns the device-layout copies of the
(frozen) weights -- fragment-tiled so that the same bytes feed both the
128x128 MFMA tile GEMM (prefill / training shapes) and the weight-streaming
decode GEMM -- the rotary tables, the KV cache objects and, for decode, a
HIP graph of the whole token step (28 x ~10 launches + head) that is replayed
per token with the position held in device memory.

Per block (parallel residual, adapters after attention/MLP):
    ln   = LayerNorm(x)
    qkv  = ln Wqkv^T                      -> rotary(q,k), K/V scattered into the cache
    ctx  = causal softmax(q k^T / 16) v   (flash kernel / decode kernel)
    a    = ctx Wout^T                     [v2: a += Wup relu(Wdn a + b) + b]
    h    = gelu_new(ln Wfc^T + b)
    m    = h Wproj^T + b
    x'   = m + Wup relu(Wdn m + b) + b + a + x     (one GEMM epilogue: bias + 3 residuals)
"""
from __future__ import annotations

import itertools
import os
import weakref
from typing import List, Optional

import torch

from . import adapters, ops
from .language_model import LMOutput
from .selection import BeamBuffers, ConstraintMode, ContrastBuffers, SelectionPlan, StepKey, TokenSelection  # noqa: F401

BF16 = torch.bfloat16
_PACK_GENS = itertools.count(1)      # LMEngine._packs_gen


def rotary_tables(rotary_dim: int, n_pos: int, device):
    """sin/cos of pos * 10000^(-2i/rotary_dim) in fp32, computed with the same
    torch expression as HF/GPT-J's create_sinusoidal_positions so the table is
    bit-identical to what the reference graph multiplies by."""
    inv_freq = 1.0 / (10000 ** (torch.arange(0, rotary_dim, 2, dtype=torch.int64).float() / rotary_dim))
    ang = torch.einsum("i,j->ij", torch.arange(n_pos, dtype=torch.int64).float(), inv_freq)
    return torch.sin(ang).to(device).contiguous(), torch.cos(ang).to(device).contiguous()


class KVCache:
    """Opaque ``past_key_values`` (reference sampling.py:81-93 only hands it back)."""

    def __init__(self, n_layer: int, B: int, H: int, Smax: int, device, ragged: bool = False):
        self.k = torch.empty(n_layer, B, H, Smax, 256, dtype=BF16, device=device)
        self.v = torch.empty(n_layer, B, H, Smax, 256, dtype=BF16, device=device)
        # next write position: one for the batch, or -- ragged (right-padded prompts of different lengths) -- one per row
        self.ragged = bool(ragged)
        self.pos_stride = 1 if self.ragged else 0                         # launch argument of every decode kernel
        self.d_pos = torch.zeros(B if self.ragged else 1, dtype=torch.int32, device=device)
        self.pos = 0                                                     # host mirror (ragged: of the largest position)
        # token-selection state of the generate() loop (device side): {step, first step at which every row emitted eos},
        # the seed of the sampling stream, the eos id the bookkeeping launch compares against
        self.sample_state = torch.tensor([0, -1], dtype=torch.int32, device=device)
        self.seed = torch.zeros(1, dtype=torch.int64, device=device)
        # per-request sampling (DESIGN.md "Per-request sampling"): one record of settings and seed per row (uint8 [B,
        # ops.SAMPLE_ROW_BYTES]; allocated by SelectionPlan.arm under a ("rows", warp) mode, written outside the captured step)
        self.sample_rows = None
        self.eos = -1
        self.history = torch.zeros(B, Smax, dtype=torch.int64, device=device)   # token selected at step s of the current loop
        self.B, self.Smax = B, Smax
        self.decode_state = None
        self.beam = None          # BeamBuffers of a beam-search loop (B = samples x num_beams rows), allocated on first use
        self.contrast = None      # ContrastBuffers of a contrastive-search loop (B = samples x top_k rows), allocated on first use
        self.prefill_x = None     # the prefill's last-block output (B, S, d), kept only for a contrastive plan to arm from
        # logits processors: the suppress ids on the device (int32 [1024], allocated on first use; its address and the NUMBER of
        # ids are launch arguments of the captured step, the ids themselves are not) and the host copy of what it holds
        self.suppress, self.suppress_ids = None, ()
        # per-row stopping: the stop table on the device (int32 [ops.STOP_TABLE_INTS]: eos ids, sequence lengths, sequence
        # tokens; allocated on first use; its address and the COUNTS are launch arguments of the captured step, its contents are
        # not), the host copy of what it holds, and the finish record int32 [B, 2] = {step the row finished at or -1, reason}
        self.stop_table, self.stop_held, self.finish = None, None, None
        # continuing from this cache (DESIGN.md "Continuing from a cache"): host copy of the per-row write positions as of host
        # position _rows_at (None: every row at self.pos), and per row the generated token not yet fed back (-1: none)
        self._rows, self._rows_at = None, 0
        self.pending = None
        self.owner = None         # weak reference to the LMEngine whose prefill filled the cache (None: not recorded)
        # token log-probabilities (DESIGN.md "Token log-probabilities"), beside the history: fp32 [B, Smax] log-probability of the
        # token selected at step s, and the n_top most probable tokens of that step (int32 / fp32 [B, Smax, n_top]); allocated on
        # first request (SelectionPlan.arm), addresses and n_top are launch arguments of the captured step
        # (lp_cols: a slot session keeps one column per token of a request's budget instead -- SlotSession sets it; 0: Smax)
        self.lp = self.top_id = self.top_lp = None
        self.lp_cols = 0
        # constrained decoding (DESIGN.md "Constrained decoding"): the trie table (int32, grown when a table outgrows it), the
        # per-row roots int32 [B] and the kernel's path cache int32 [B, 64]; allocated on first use (SelectionPlan.arm).
        # Addresses and the table's capacity are launch arguments of the captured step, the contents are not; trie_held is the
        # ConstraintMode whose table and roots the buffers hold
        self.trie_table = self.trie_roots = self.trie_path = self.trie_held = None
        # request streams (DESIGN.md "Request streams"): the per-row window int32 [B, 2] = {begin column, token budget} and the RING
        # token history int64 [B, ring_cols] of a slot session (SlotSession sets ring_cols, SelectionPlan.arm allocates); their
        # addresses and ring_cols are launch arguments of the captured step
        self.slot_table, self.ring, self.ring_cols = None, None, 0
        # shared session prefix (DESIGN.md "Shared session prefix"; SlotSession sets it): ONE copy of the K / V of prefix_P positions,
        # [L, 1, H, prefix_P, 256], in front of every row -- k / v then hold the rows' OWN positions, absolute position p at own index
        # p - prefix_P, while d_pos and pos stay absolute.  None / 0: every position of a row is its own
        self.prefix_k = self.prefix_v = None
        self.prefix_P = 0
        # speculative decoding (DESIGN.md "Speculative decoding"): T -> the decode state of the step that runs T rows per sequence
        # (scratch for B * T rows, its own captured graphs, the loop's bookkeeping buffers), apart from decode_state: a plain call
        # on this cache replays its own graphs untouched
        self.spec = {}

    def alloc_trie(self, n_ints: int):
        """The constraint's buffers for a table of ``n_ints`` (kept when it fits); steps captured on other buffers are dropped."""
        if self.trie_table is not None and self.trie_table.numel() >= n_ints:
            return
        dev = self.k.device
        self.trie_table = torch.zeros(max(4096, 2 * n_ints), dtype=torch.int32, device=dev)
        self.trie_held = None
        if self.trie_roots is None:
            self.trie_roots = torch.zeros(self.B, dtype=torch.int32, device=dev)
            self.trie_path = ops.trie_path(self.B, dev)
        self._drop_graphs(lambda key: key.constrained)

    def alloc_logprobs(self, n_top: int):
        """The per-step log-probability buffers for ``n_top`` alternatives per token (kept when they already have that shape);
        steps captured on other buffers are dropped."""
        cols = self.lp_cols or self.Smax
        if self.lp is not None and self.lp.shape[1] == cols and self.top_id.shape[2] == n_top:
            return
        dev = self.k.device
        self.lp = torch.zeros(self.B, cols, dtype=torch.float32, device=dev)
        self.top_id = torch.zeros(self.B, cols, n_top, dtype=torch.int32, device=dev)
        self.top_lp = torch.zeros(self.B, cols, n_top, dtype=torch.float32, device=dev)
        self._drop_graphs(lambda key: key.n_top is not None)

    def __len__(self):
        return self.k.shape[0]

    def rows_pos(self) -> torch.Tensor:
        """Host int64 [B]: the next write position of every row (no device sync: every step since the last set advanced all rows)."""
        if self._rows is None:
            return torch.full((self.B,), self.pos, dtype=torch.int64)
        return self._rows + (self.pos - self._rows_at)

    def _drop_graphs(self, which=lambda key: True):
        """Forget the captured steps whose StepKey ``which`` selects (by default all of them)."""
        graphs = self.decode_state.graphs if self.decode_state is not None else {}
        for key in [k for k in graphs if which(k)]:
            del graphs[key]
        for st in self.spec.values():         # (a speculative step's key: its StepKey, the token limit, the lookup width)
            for key in [k for k in st.graphs if which(k[0])]:
                del st.graphs[key]

    def set_rows(self, pos, pending=None):
        """Row b's next write position becomes pos[b] (host ints; the cache turns ragged), its not-yet-fed token pending[b] (-1 none)."""
        pos = torch.as_tensor(pos, dtype=torch.int64).cpu().view(-1)
        assert pos.numel() == self.B
        if not self.ragged:           # pos_stride and the d_pos buffer are launch arguments of the captured token step
            self.ragged, self.pos_stride = True, 1
            self.d_pos = torch.zeros(self.B, dtype=torch.int32, device=self.k.device)
            self._drop_graphs()
        self.d_pos.copy_(pos.to(torch.int32), non_blocking=True)
        self._rows, self.pos = pos.clone(), int(pos.max())
        self._rows_at = self.pos
        self.pending = None if pending is None else torch.as_tensor(pending, dtype=torch.int64).cpu().view(-1).clone()

    def grow(self, Smax: int):
        """Re-allocate for Smax positions, keeping the written ones; graphs captured on the old buffers are dropped."""
        if Smax <= self.Smax:
            return
        used = min(self.Smax, int(self.rows_pos().max()))
        for name in ("k", "v"):
            old = getattr(self, name)
            new = torch.empty(*old.shape[:3], Smax, old.shape[4], dtype=old.dtype, device=old.device)
            new[:, :, :, :used].copy_(old[:, :, :, :used])
            setattr(self, name, new)
        self.history = torch.zeros(self.B, Smax, dtype=torch.int64, device=self.k.device)
        self.Smax = Smax
        self.beam = self.contrast = None
        self.spec = {}
        self._drop_graphs()
        if self.lp is not None:           # one column per history column
            self.alloc_logprobs(self.top_id.shape[2])

    def expand(self, n: int) -> "KVCache":
        """A new cache in which every row appears n times in a row (sample-major, row b -> rows b n .. b n + n - 1): one prompt
        cached once, continued by n different inputs.  Only the written positions are copied."""
        if not isinstance(n, int) or n < 1:
            raise ValueError(f"expand(n) takes an integer n >= 1, got {n!r}")
        rows = self.rows_pos()
        used = min(self.Smax, int(rows.max()))
        out = KVCache(len(self), self.B * n, self.k.shape[2], self.Smax, self.k.device, ragged=True)
        out.k[:, :, :, :used].copy_(self.k[:, :, :, :used].repeat_interleave(n, dim=1))
        out.v[:, :, :, :used].copy_(self.v[:, :, :, :used].repeat_interleave(n, dim=1))
        out.eos, out.owner = self.eos, self.owner
        out.set_rows(rows.repeat_interleave(n), None if self.pending is None else self.pending.repeat_interleave(n))
        return out


class _Layer:
    pass


class LMEngine(TokenSelection):
    def __init__(self, lm):
        cfg = lm.config
        self.cfg = cfg
        dev = lm.lm_head.weight.device
        if dev.type != "cuda":
            raise ops.L.MagmaHipError("the MAGMA LM runs on MI355X only: move the model to a GPU (no CPU fallback)")
        self.device = dev
        self.d, self.H, self.L = cfg.hidden_size, cfg.num_heads, cfg.num_layers
        if self.d != self.H * 256:
            raise ValueError("the attention kernels are specialised for head_dim = 256 (GPT-J)")
        self.eps = cfg.layer_norm_epsilon
        self.wte = lm.transformer.wte.weight.detach()
        if self.wte.dtype != BF16:
            self.wte = self.wte.to(BF16)
        self.wte = self.wte.contiguous()
        self.V = lm.lm_head.weight.shape[0]
        self.layers: List[_Layer] = []
        f32 = lambda t: t.detach().float().contiguous()  # noqa: E731
        from .adapters import ParallelAdapter
        for blk in lm.transformer.h:
            ly = _Layer()
            attn = blk.attn
            ly.attn_adapter = None
            # parallel adapters (reference adapters.py:42-92) read the block INPUT (ln_1 output) instead of the wrapped
            # module's output and are scaled by adapter_scale: *_par = fp32 [d] vector holding the scale, else None
            ly.attn_par = ly.mlp_par = None
            # adapter options (reference adapters.py:11-24): *_act = epilogue code of the bottleneck activation, *_ad_ln =
            # (gamma, beta, eps) of the LayerNorm in front of the down-projection or None
            ly.attn_act = ly.mlp_act = ops.MG_ACT_RELU
            ly.attn_ad_ln = ly.mlp_ad_ln = None
            if isinstance(attn, ParallelAdapter):    # ParallelAdapterWrapper
                ly.attn_adapter, ly.attn_act, ly.attn_ad_ln = self._pack_adapter(attn)
                ly.attn_par = torch.full((self.d,), attn.scale_value(), dtype=torch.float32, device=dev)
                attn = attn.module
            elif hasattr(attn, "attn_block"):        # AdapterWrapper (v2)
                ly.attn_adapter, ly.attn_act, ly.attn_ad_ln = self._pack_adapter(attn)
                attn = attn.attn_block
            a = attn.attention
            ly.out = ops.PackedLinear(a.out_proj.weight)
            mlp = blk.mlp
            ly.mlp_adapter = None
            if isinstance(mlp, ParallelAdapter):
                ly.mlp_adapter, ly.mlp_act, ly.mlp_ad_ln = self._pack_adapter(mlp)
                ly.mlp_par = torch.full((self.d,), mlp.scale_value(), dtype=torch.float32, device=dev)
                mlp = mlp.module
            elif isinstance(mlp, torch.nn.Sequential):  # Sequential(mlp, Adapter)  (reference magma.py:143-149)
                ly.mlp_adapter, ly.mlp_act, ly.mlp_ad_ln = self._pack_adapter(mlp[1])
                mlp = mlp[0]
            # qkv and fc_in read the same LayerNorm output: ONE operand [q | k | v | fc_in] (bias: zeros | b_fc) for the fused
            # prefill GEMM; ly.qkv / ly.fc_in are row ranges of it that share its storage
            d3 = 3 * self.d
            fcb = mlp.c_fc.bias.detach().float()
            ly.in_cat = ops.PackedLinear(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, mlp.c_fc.weight], dim=0),
                                         bias=torch.cat([torch.zeros(d3, dtype=torch.float32, device=dev), fcb]))
            ly.qkv = ly.in_cat.rows(0, d3)
            ly.fc_in = ly.in_cat.rows(d3, ly.in_cat.N, bias=fcb.contiguous())
            ly.fc_out = ops.PackedLinear(mlp.c_proj.weight, mlp.c_proj.bias)
            ly.ln_g, ly.ln_b = f32(blk.ln_1.weight), f32(blk.ln_1.bias)
            ly.dec_in = None      # decode-only fused [qkv | fc_in] operand with ln_1 folded in (built lazily)
            # lazily built operands, None until built (whether a block HAS one is _block_kind's answer, not the field's):
            # [W_out | W_up] (_ensure_out_up), [W_up_mlp | W_up_attn] (_adapter_up_cat), [W_fc_out ; W_dn W_fc_out]
            # (_fold_adapter_down), the e4m3 prefill copies by projection name (_fp8_weight), the W8A16 / W4A16 decode operands
            ly.out_up = ly.up_cat = ly.fc_dn = ly.w8 = ly.w4 = None
            ly.fp8 = {}
            ly._src = (a, mlp)
            self.layers.append(ly)
        self.lnf_g, self.lnf_b = f32(lm.transformer.ln_f.weight), f32(lm.transformer.ln_f.bias)
        self.head = ops.PackedLinear(lm.lm_head.weight, lm.lm_head.bias)
        self.Vp = ops.ceil_to(self.V, 8)
        self.sin_t, self.cos_t = rotary_tables(cfg.rotary_dim, cfg.max_position_embeddings, dev)
        self.rot = cfg.rotary_dim
        self.head_dec = self.head_w8 = self.head_w4 = None
        self._lm_head = lm.lm_head
        # The adapter operands are copies of TRAINED weights.  _packs_epoch: adapters._WEIGHTS_EPOCH (bumped by every writer that goes
        # round torch: the optimizer step, Magma.invalidate_packed) when they were last packed -- _current_packs repacks when it
        # moved.  _packs_gen: one number per set of packs, unique across engines; a cache's captured steps hold the raw addresses of
        # one set and are dropped (decode) when the number differs.
        self._blocks = lm.transformer.h
        self._packs_epoch, self._packs_gen = adapters._WEIGHTS_EPOCH, next(_PACK_GENS)
        # (B, Smax, ragged) -> KVCache + the decode graphs captured on it, least recently used first; at most _cache_pool_max
        # entries (MAGMA_CACHE_POOL, default 4; 0 = no pooling: every generate() call allocates its cache and keeps nothing)
        self._cache_pool = {}
        self._cache_pool_max = int(os.environ.get("MAGMA_CACHE_POOL", "4"))
        if self._cache_pool_max < 0:
            raise ValueError(f"MAGMA_CACHE_POOL must be an integer >= 0 (0 = no pooling), got {self._cache_pool_max}")
        # fp8 operands for the prefill / forward GEMMs (BASELINE config 5): None | "attn" (QKV, out_proj, adapters)
        # | "all" (+ fc_in, fc_out).  bf16 stays the default: it is what the parity tests and the headline use.
        self.fp8_mode = os.environ.get("MAGMA_FP8") or None
        self.fp8_attn = os.environ.get("MAGMA_FP8_ATTN", "1") == "1"     # with fp8_mode: QK^T / PV of the cache-less forward in e4m3 too
        # scaling of the fp8 operands: "row" = one fp32 scale per activation row / weight output channel (any tile kernel), "mx" =
        # OCP MX, one E8M0 scale per 32 K-elements of both operands, applied by the MFMA itself (both tile kernels)
        self.fp8_scaling = os.environ.get("MAGMA_FP8_SCALING", "row")
        if self.fp8_scaling not in ("row", "mx"):
            raise ValueError("MAGMA_FP8_SCALING must be 'row' or 'mx'")
        # W8A16 decode: e4m3 weights (per-output-channel scales) widened to bf16 in registers by the weight-streaming
        # GEMVs -> half the bytes per token step.  Changes the numerics (weight quantisation), so it is opt-in.
        self.decode_w8 = os.environ.get("MAGMA_DECODE_W8", "0") == "1"
        # W4A16 decode: OCP MXFP4 weights (e2m1 codes, one E8M0 scale per 32 K-elements), widened the same way -> 4.25 bits per
        # weight.  Opt-in for the same reason, and exclusive with W8A16 (_quantised_decode: both set is an error).
        self.decode_w4 = os.environ.get("MAGMA_DECODE_W4", "0") == "1"
        self._quantised_decode()
        # Lossless decode packing: the bf16 token step streams its weights as 13.25-bit twins (ops.DecodePack, built with the decode
        # operands) that the GEMVs widen back to the SAME bf16 bits in registers -- identical logits, 0.83x the bytes, about 10 GB
        # more HBM for the benchmark model.  Read when the decode operands are built; the W8A16 / W4A16 steps and B > 16 ignore it.
        self.decode_pack = os.environ.get("MAGMA_DECODE_PACK", "1") == "1"
        self._dec_in_variant = int(os.environ.get("MAGMA_DEC_IN_VARIANT", "0"))   # tuning knob: nt | waves<<4 | kc<<8
        self._dec_dn_variant = int(os.environ.get("MAGMA_DEC_DN_VARIANT", "0"))   # the same for the adapter-down and the
        self._dec_cat_variant = int(os.environ.get("MAGMA_DEC_CAT_VARIANT", "0"))  # [W_out | W_up] launches of the v1 block
        self.group_launches = os.environ.get("MAGMA_DECODE_GROUPED", "1") == "1"
        # MAGMA_DECODE_FOLD -- how the adapter of a MAGMA_v1 block is laid over the block's launches (round 4):
        #   0  four launches as in rounds 1-3: [ln_1+qkv+fc_in] -> [attention || fc_out] -> [out_proj || adapter-down] -> [adapter-up]
        #   2  (default) the up-projection shares a launch with out_proj as ONE GEMV over the concatenated input [ctx | t] against
        #      [W_out | W_up]:  ... -> [attention || fc_out] -> [adapter-down] -> [[W_out | W_up]]: x' = that + b_up + m + x.  Same
        #      bytes, same launch count, 2.500 against 2.522-2.528 ms per token (the 8 MB up-projection no longer pays a
        #      launch of its own; adapter-down alone costs what the co-launch with out_proj hid).
        #   1  THREE launches: the down-projection multiplied through fc_out offline -- t = relu(W_dn m + b_dn), m = W_fc h + b_fc,
        #      so t = relu((W_dn W_fc) h + (W_dn b_fc + b_dn)), a second output segment of the fc_out launch (+25 MB per block).
        #      Parity-green (re-association only: tests/test_fullwidth_gpu.py) and SLOWER, 2.70 ms per token: the co-launch grows
        #      from 256 to 320 weight tiles of 512 KB on 256 CUs and takes 41.4 us instead of 29.6 (a quarter of the CUs stream two
        #      tiles), more than the merged [W_out | W_up] launch saves (9.7 us for 13.2 + 5.0).  profiles/r04_decode_block_variants.txt
        # The reference forms the same sum (reference adapters.py:38-39) in another association order.
        self.fold_dn = int(os.environ.get("MAGMA_DECODE_FOLD", "2"))
        self.fuse_in = os.environ.get("MAGMA_PREFILL_FUSE_IN", "1") == "1"      # [qkv | fc_in] as one prefill GEMM
        self.cat_up = os.environ.get("MAGMA_PREFILL_CAT", "1") == "1"           # out_proj + adapter-up as one GEMM over [ctx | t]

    @staticmethod
    def _pack_adapter(mod):
        """((down, up) packed, activation code, (gamma, beta, eps) | None) of an Adapter-like module, whatever its options."""
        from .adapters import activation_codes
        code, _, _ = activation_codes(mod.act)
        ln = None
        if mod.ln is not None:
            ln = (mod.ln.weight.detach().float().contiguous(), mod.ln.bias.detach().float().contiguous(), float(mod.ln.eps))
        return (ops.PackedLinear(mod.down.weight, mod.down.bias), ops.PackedLinear(mod.up.weight, mod.up.bias)), code, ln

    @staticmethod
    def _epi_act(code):
        """Epilogue code of a bottleneck activation: torch.nn.GELU() (erf) is not an epilogue -- the GEMM runs without activation
        and _act_fix applies it as its own pass."""
        return ops.MG_ACT_NONE if code == ops.MG_ACT_GELU_ERF else code

    @staticmethod
    def _act_fix(t, code):
        return ops.gelu_erf(t, out=t) if code == ops.MG_ACT_GELU_ERF else t

    @staticmethod
    def _ad_in(ln, x, out=None):
        """Input of an adapter's down-projection: x, or LayerNorm(x) for an adapter built with add_layernorm."""
        return x if ln is None else ops.layernorm(x, ln[0], ln[1], ln[2], out=out)

    def _adapter(self, G_dn, G_up, pair, act, ln, x_in, par, residuals, t=None, ln_out=None, out=None):
        """Bottleneck adapter after or beside a projection:  out = up(act(down([LayerNorm] x_in))) [* par] + residuals.
        ``pair`` = (down, up) packed; ``act`` the activation code (erf-GELU runs as its own pass over t); ``ln`` the adapter's
        (gamma, beta, eps) or None; ``x_in`` the wrapped projection's output, or -- parallel adapters, ``par`` = their scale vector
        -- the block's ln_1 output.  ``G_dn`` / ``G_up`` (x, w, **epilogue) launch the two GEMMs: the decode step passes its GEMV
        (or tile GEMM) twice and its scratch buffers ``t`` / ``ln_out`` / ``out``; the prefill passes _linear under the
        projections' fp8 names (a parallel up-projection stays on ops.gemm) and lets the GEMMs allocate."""
        dn, up = pair
        kw = {}
        if par is not None:
            kw["scale"], up = self._par_up(up, par)
        t = self._act_fix(G_dn(self._ad_in(ln, x_in, out=ln_out), dn, out=t, act=self._epi_act(act)), act)
        return G_up(t, up, out=out, residuals=residuals, **kw)

    def _fold_pack(self, cls, w, b, gamma, beta, split=None):
        """LayerNorm(gamma, beta) folded into [w; b] (ops.fold_layernorm), packed as ``cls`` (PackedLinear | PackedLinearW8 | PackedLinearW4).
        ``split``: the bias of the output columns >= split goes to .bias_b (second segment of a split launch).  The e4m3 pack
        takes the fold's column sums from its DEQUANTISED weights, so that  rstd*(acc*scale - mean*colsum)  stays exact for what
        the kernel multiplies; the MXFP4 pack does the same (fold first, then quantise)."""
        w2, b2, cs = ops.fold_layernorm(w, b, gamma, beta)
        lin = cls(w2, bias=b2 if split is None else b2[:split])
        if split is not None:
            lin.bias_b = b2[split:].contiguous()
        lin.colsum = cs if cls is ops.PackedLinear else lin.dequant().sum(1).contiguous()
        return lin

    def _fold_dec_in(self, cls, ly):
        """[q | k | v | fc_in] with ln_1 folded in: [3d+ff, d], bias zeros | b_fc (.bias over the qkv columns, .bias_b over fc_in)."""
        a, mlp = ly._src
        d3 = 3 * self.d
        w = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, mlp.c_fc.weight], dim=0)
        b = torch.cat([torch.zeros(d3, device=self.device), mlp.c_fc.bias.detach().float()])
        return self._fold_pack(cls, w, b, ly.ln_g, ly.ln_b, split=d3)

    def _fold_head(self, cls):
        return self._fold_pack(cls, self._lm_head.weight, self._lm_head.bias, self.lnf_g, self.lnf_b)

    def _ensure_decode_packs(self):
        """Decode operands with the LayerNorms folded in (frozen gamma/beta): per layer one
        fused [3d+ff, d] matrix W' = [Wqkv;Wfc]*gamma whose single weight-streaming launch
        produces qkv and gelu(fc_in) from the raw residual stream (no LayerNorm launch, one
        GEMV instead of two); ln_f is folded into lm_head the same way."""
        if self.head_dec is not None:
            return
        for ly in self.layers:
            ly.dec_in = self._fold_dec_in(ops.PackedLinear, ly)
            self._fold_adapter_down(ly)
            if self.fold_dn in (1, 2):
                self._ensure_out_up(ly)          # built HERE, never inside a token step (no allocation under hipGraph capture)
        self.head_dec = self._fold_head(ops.PackedLinear)
        for ly in self.layers:
            self._attach_decode_twins(ly)
        if self.decode_pack:
            ops.attach_decode_pack(self.head_dec)

    def _attach_decode_twins(self, ly):
        """decode_pack: the lossless 13.25-bit twins (ops.DecodePack) of the weight-streaming operands of a "fold2" / "grouped" block --
        the token step then streams 0.83x the bytes and computes the same bits.  An operand that already has its twin keeps it
        (frozen weights are packed once per model); repack_adapters calls this again for the adapter operands it rebuilt.  Built
        with the decode operands, never inside a token step."""
        if not self.decode_pack or self.decode_w8 or self.decode_w4:     # the quantised steps stream their own operands
            return
        kind = self._block_kind(ly, False, False, self.fold_dn, self.group_launches)
        if kind == "fold2":
            operands = (ly.dec_in, ly.fc_out, ly.mlp_adapter[0], ly.out_up)
        elif kind == "grouped":
            operands = (ly.dec_in, ly.fc_out, ly.out) + tuple(ly.mlp_adapter)
        else:
            return
        for p in operands:
            if p is not None:
                ops.attach_decode_pack(p)

    def decode_pack_share(self) -> float:
        """Share of the token step's weight bytes (bf16 count, B <= 16, current switches) that is streamed packed: operands with a
        twin, less their escaped row tiles."""
        self._ensure_decode_packs()
        packed = total = 0
        kinds = [self._block_kind(ly, False, False, self.fold_dn, self.group_launches) for ly in self.layers]
        for ly, kind in zip(self.layers, kinds):
            if kind == "fold2":
                operands = [ly.dec_in, ly.fc_out, ly.mlp_adapter[0], ly.out_up]
            elif kind == "fold1":
                operands = [ly.dec_in, ly.fc_dn, ly.out_up]
            else:
                operands = [ly.dec_in, ly.fc_out, ly.out] + [p for pair in (ly.mlp_adapter, ly.attn_adapter) if pair for p in pair]
            for p in operands + ([self.head_dec] if ly is self.layers[-1] else []):
                total += p.ft.numel()
                pk = getattr(p, "pk", None)
                if pk is not None:
                    packed += p.ft.numel() * (pk.ntiles - pk.escaped) // pk.ntiles
        return packed / max(total, 1)

    def _block_kind(self, ly, wide=False, w8=False, fold_dn=0, group=True) -> str:
        """Which launch sequence (_block_<kind>) the token step runs for this layer: "wide" | "fold2" | "fold1" | "grouped" | "v2" |
        "generic" -- the ONE place that tells the block shapes apart (table: DESIGN.md, "The six block kinds").  A MAGMA_v1 block
        (v1 below) is the 'normal' MLP adapter with a plain ReLU bottleneck -- what the folds are written for -- and every K a
        multiple of 128; a fold that does not apply, and W8A16 always, falls to the four-launch "grouped" block."""
        if wide:
            return "wide"
        if (not group or ly.mlp_adapter is None or ly.mlp_par is not None or ly.attn_par is not None or ly.mlp_ad_ln is not None
                or ly.mlp_act == ops.MG_ACT_GELU_ERF):
            return "generic"
        dn, up = ly.mlp_adapter
        k128 = all(p.Kp % 128 == 0 for p in (ly.fc_out, ly.out, dn))
        if ly.attn_adapter is None:
            if not k128:
                return "generic"
            v1 = ly.mlp_act == ops.MG_ACT_RELU and not (dn.N % 16 or (self.d + dn.N) % 128 or dn.K != self.d or up.K != dn.N
                                                        or up.Kp != up.K)
            if v1 and not w8 and fold_dn == 2:
                return "fold2"
            if v1 and not w8 and fold_dn == 1 and ly.fc_dn is not None:
                return "fold1"
            return "grouped"
        dn_a, up_a = ly.attn_adapter
        if ly.attn_ad_ln is not None or ly.attn_act == ops.MG_ACT_GELU_ERF:       # a pass of its own after the down-projection
            return "generic"
        cat = dn.N == up.K == up.Kp and dn_a.N == up_a.K == up_a.Kp and (up.K + up_a.K) % 128 == 0
        return "v2" if cat and k128 and dn_a.Kp % 128 == 0 else "generic"

    def _v1_block(self, ly) -> bool:
        """MAGMA_v1 block shape (_block_kind): the blocks that have a [W_out | W_up] operand."""
        return self._block_kind(ly, fold_dn=2) == "fold2"

    def _ensure_out_up(self, ly):
        """[W_out | W_up] (d rows over K = d + r, bias b_up) of a MAGMA_v1 block -- the operand of the ONE GEMM / GEMV that
        replaces out_proj and the adapter's up-projection (prefill / forward blocks and the decode step) -- or None where a
        block does not have that shape.  Built with the decode operands (_ensure_decode_packs / repack_adapters), when a token
        step is planned (_ensure_decode_state) or on the first prefill that wants it; dropped AND rebuilt by repack_adapters (it
        contains W_up), whose new _packs_gen retires every token step captured against the old one.  It is a SECOND copy of
        W_out (42 MB per block, 1.2 GB at 28 blocks): ly.out stays for the paths that still read it (fp8 modes,
        MAGMA_PREFILL_CAT=0 / MAGMA_DECODE_FOLD=0, attention adapters)."""
        if ly.out_up is None and self._v1_block(ly):
            a, _ = ly._src
            up = ly.mlp_adapter[1]
            w_up = ops.PackedLinear.untile(up.ft)[: up.N, : up.K]
            ly.out_up = ops.PackedLinear(torch.cat([a.out_proj.weight.detach().to(BF16), w_up], dim=1), bias=up.bias)
        return ly.out_up

    def _fold_adapter_down(self, ly):
        """Decode-only operand of the three-launch block (MAGMA_DECODE_FOLD=1), or None:
          ly.fc_dn = [W_fc_out ; W_dn W_fc_out]   (d + r rows over K = ff;  bias b_fc | W_dn b_fc + b_dn)"""
        ly.fc_dn = None
        if self.fold_dn != 1 or not self._v1_block(ly):
            return
        dn, _ = ly.mlp_adapter
        _, mlp = ly._src
        w_fc, b_fc = mlp.c_proj.weight.detach().float(), mlp.c_proj.bias.detach().float()
        w_dn = ops.PackedLinear.untile(dn.ft)[: dn.N, : dn.K].float()
        ly.fc_dn = ops.PackedLinear(torch.cat([mlp.c_proj.weight.detach().to(BF16), (w_dn @ w_fc).to(BF16)], dim=0), bias=b_fc)
        ly.fc_dn.bias_b = (w_dn @ b_fc + dn.bias).contiguous()

    # the quantised decode modes: engine switch -> (name, weight class, K every operand must be a multiple of, layer / head field)
    _QUANT_DECODE = {"decode_w8": ("W8A16", "PackedLinearW8", 1024, "w8", "head_w8"),
                     "decode_w4": ("W4A16", "PackedLinearW4", 512, "w4", "head_w4")}

    def _quantised_decode(self):
        """The active quantised decode mode as its _QUANT_DECODE row, or None (bf16 weights)."""
        if self.decode_w8 and self.decode_w4:
            raise ValueError("decode_w8 (MAGMA_DECODE_W8) and decode_w4 (MAGMA_DECODE_W4) are both set: one weight format per token step")
        for switch, row in self._QUANT_DECODE.items():
            if getattr(self, switch):
                return row
        return None

    def _ensure_decode_packs_q(self, mode):
        """Quantised copies (``mode``: a _QUANT_DECODE row) of every decode operand (same LayerNorm folds, _fold_pack).  An operand
        whose K the format's kernel does not take has no copy (None): _plan_decode refuses the step that would need it."""
        _, cls, kmod, field, head = mode
        cls = getattr(ops, cls)
        if getattr(self, head) is not None or self._quant_misfit(mode) is not None:
            return
        for ly in self.layers:
            a, mlp = ly._src
            q = _Layer()
            q.dec_in = self._fold_dec_in(cls, ly)
            q.out = cls(a.out_proj.weight)
            q.fc_out = cls(mlp.c_proj.weight, mlp.c_proj.bias)
            self._quantised_adapters(q, ly, cls, kmod)
            setattr(ly, field, q)
        setattr(self, head, self._fold_head(cls))

    def _quant_misfit(self, mode):
        """Why the FROZEN projections have no operand in this quantised format (their K is d or d_ff), or None.  Nothing is
        packed then; _plan_decode hands the reason to st.refusal."""
        name, _, kmod = mode[:3]
        bad = sorted({k for ly in self.layers for k in (self.d, ly.fc_out.K) if k % kmod})
        if bad:
            return f"{name} decode needs every projection's K to be a multiple of {kmod} (this model has K = {', '.join(map(str, bad))})"
        return None

    def _quantised_adapters(self, q, ly, cls, kmod):
        """The adapter projections of ``ly`` as ``cls`` into the layer's quantised operand set ``q``."""
        unpacked = lambda p: ops.PackedLinear.untile(p.ft)[: p.N, : p.K]  # noqa: E731
        q.mlp_adapter = None
        if ly.mlp_adapter is not None:
            # (the up-projection alone is only used by the MAGMA_v1 step; in MAGMA_v2 -- K = 512 -- it lives in up_cat below)
            q.mlp_adapter = tuple(cls(unpacked(p), p.bias) if p.K % kmod == 0 else None for p in ly.mlp_adapter)
        # MAGMA_v2 (attention AND mlp adapters): the attention adapter's down-projection and the concatenated up-projection
        q.attn_adapter = q.up_cat = None
        cat = self._adapter_up_cat(ly)
        if cat is not None and cat.K % kmod == 0:
            q.attn_adapter = (cls(unpacked(ly.attn_adapter[0]), ly.attn_adapter[0].bias),)
            q.up_cat = cls(unpacked(cat), cat.bias)

    def _ensure_decode_packs_w8(self):
        """e4m3 copies of every decode operand."""
        self._ensure_decode_packs_q(self._QUANT_DECODE["decode_w8"])

    def _ensure_decode_packs_w4(self):
        """MXFP4 copies of every decode operand."""
        self._ensure_decode_packs_q(self._QUANT_DECODE["decode_w4"])

    def repack_adapters(self, lm=None):
        """Refresh only the (trainable) adapter operands after optimizer steps; the
        12 GB of frozen weights keep their packed copies.  Every operand that contains an adapter weight is a NEW tensor
        afterwards and the old ones go back to the allocator: a token step captured before (on a pooled cache or on one the
        caller holds) points at freed memory.  No cache is visited here: the new _packs_gen makes _ensure_decode_state drop a
        cache's captured steps before decode() would replay one.  Called by MagmaEngine.eval() and, for every other writer
        that bumps the weights epoch, by _current_packs; ``lm`` defaults to the model this engine was built from."""
        self._packs_epoch, self._packs_gen = adapters._WEIGHTS_EPOCH, next(_PACK_GENS)
        for ly, blk in zip(self.layers, self._blocks if lm is None else lm.transformer.h):
            if ly.attn_adapter is not None:
                ly.attn_adapter, ly.attn_act, ly.attn_ad_ln = self._pack_adapter(blk.attn)
                if ly.attn_par is not None:           # scaled_parallel: the scale is a trained parameter too
                    ly.attn_par = torch.full((self.d,), blk.attn.scale_value(), dtype=torch.float32, device=ly.attn_par.device)
            if ly.mlp_adapter is not None:
                par = ly.mlp_par is not None
                ly.mlp_adapter, ly.mlp_act, ly.mlp_ad_ln = self._pack_adapter(blk.mlp if par else blk.mlp[1])
                if par:
                    ly.mlp_par = torch.full((self.d,), blk.mlp.scale_value(), dtype=torch.float32, device=ly.mlp_par.device)
            ly.fp8 = {}
            # [W_out | W_up], [W_up_mlp | W_up_attn] and the folded down-projection contain the adapter weights: what was built
            # is rebuilt now, not inside the next token step (a planned step reads the fields, it does not build them)
            had_out_up, had_up_cat = ly.out_up is not None, ly.up_cat is not None
            ly.up_cat = ly.out_up = ly.fc_dn = None
            if self.head_dec is not None:
                self._fold_adapter_down(ly)
            if had_out_up or (self.head_dec is not None and self.fold_dn in (1, 2)):
                self._ensure_out_up(ly)
            if had_up_cat:
                self._adapter_up_cat(ly)
            if self.head_dec is not None:
                self._attach_decode_twins(ly)          # the rebuilt adapter operands get new twins; the frozen ones keep theirs
            for _, cls, kmod, field, _ in self._QUANT_DECODE.values():
                if getattr(ly, field) is not None:     # the quantised decode operands hold copies of the adapter projections
                    self._quantised_adapters(getattr(ly, field), ly, getattr(ops, cls), kmod)

    def _current_packs(self):
        """Entry of every pass over the blocks (_blocks_prefill, decode): the adapter operands are those of the weights as they are
        NOW -- repacked if the weights epoch moved since they were packed (generate() after step() without eval()).  The epoch is
        process-wide: a write to another model repacks this one's adapters once more, to the values they had."""
        if self._packs_epoch != adapters._WEIGHTS_EPOCH:
            self.repack_adapters()

    @staticmethod
    def _par_up(up, par):
        """(scale vector, packed up-projection whose bias is pre-multiplied by the scale) of a parallel adapter:
        the epilogue computes acc*scale[n] + bias[n], the reference (acc + b_up) * adapter_scale."""
        key = "_par_scaled"
        sc = up.__dict__.get(key)
        if sc is None:
            sc = up.__dict__[key] = ops.PackedLinear.__new__(ops.PackedLinear)
            sc.__dict__.update(up.__dict__)
            sc.bias = None if up.bias is None else (up.bias * par[: up.N]).contiguous()
        return par, sc

    def _adapter_up_cat(self, ly):
        """[W_up_mlp | W_up_attn] along K (bias = sum) for blocks that carry both adapters (_block_kind "v2"), or None.  Built when
        a token step is planned or with the W8A16 operands, never inside a step."""
        if ly.up_cat is None and self._block_kind(ly) == "v2":
            up_m, up_a = ly.mlp_adapter[1], ly.attn_adapter[1]
            w = torch.cat([ops.PackedLinear.untile(up_m.ft)[: up_m.N, : up_m.K], ops.PackedLinear.untile(up_a.ft)[: up_a.N, : up_a.K]], dim=1)
            ly.up_cat = ops.PackedLinear(w, bias=up_m.bias + up_a.bias)
        return ly.up_cat

    # ---- fp8 operand path (config 5) ----------------------------------------------------------------
    def _fp8_weight(self, ly, name: str, lin):
        """e4m3 copy (per-output-channel scales) of a packed bf16 weight, made on first use."""
        mx = self.fp8_scaling == "mx"
        w8 = ly.fp8.get(name)
        if w8 is None or isinstance(w8, ops.PackedLinearMX) != mx:
            w = ops.PackedLinear.untile(lin.ft)[: lin.N, : lin.K] if lin.ft is not None else lin.rm[: lin.N, : lin.K]
            w8 = ly.fp8[name] = (ops.PackedLinearMX if mx else ops.PackedLinearFP8)(w, lin.bias)
        return w8

    def _quantize(self, x):
        return ops.quantize_mx_fp8(x) if self.fp8_scaling == "mx" else ops.quantize_rows_fp8(x)

    def _linear(self, ly, name, lin, x, xq=None, **kw):
        """x @ lin^T through the bf16 tile GEMM, or -- when this projection is in the active fp8 set -- through the
        fp8 MFMA on a freshly quantised (per-row scale) copy of x.  ``xq`` passes an already quantised x."""
        on = self.fp8_mode == "all" or (self.fp8_mode == "attn" and name not in ("fc_in", "fc_out"))
        if not on or lin.K % 16:
            return ops.gemm(x, lin, **kw)
        q, sc = xq if xq is not None else self._quantize(x)
        if self.fp8_scaling == "mx":
            return ops.gemm_mx_fp8(q, sc, self._fp8_weight(ly, name, lin), **kw)
        return ops.gemm_fp8(q, sc, self._fp8_weight(ly, name, lin), **kw)

    # ------------------------------------------------------------------ API
    def forward(self, input_ids=None, inputs_embeds=None, labels=None, use_cache=False, past_key_values=None,
                output_hidden_states=False, cache_hint: Optional[int] = None, reuse_cache: bool = False,
                return_logits: bool = False, sampling=None, eos_token: Optional[int] = None,
                seed: Optional[int] = None, feed_back: bool = False, lengths=None, beam=None, processors=None,
                stop=None, logprobs=None, constraint=None, guidance=None, plan=None) -> LMOutput:
        """``plan`` (a SelectionPlan): selection_plan's checked form of the seven selection keywords that follow, INSTEAD of them.
        ``beam`` = (num_beams, length_penalty, early_stopping, max_steps): beam-search token selection (the rows are
        samples x num_beams, sample-major; DESIGN.md "Beam search") instead of ``sampling``.  Followed by (num_beam_groups > 1,
        diversity_penalty): diverse beam search (rows sample-major, then group-major; DESIGN.md "Diverse beam search").
        ``processors`` (sampling.check_processor_args' dict, or None): the logits processors in front of whichever selection
        runs (DESIGN.md "Logits processors").  The first token is selected from a processed COPY of the prefill / extend
        logits (``.logits`` stays raw); a cached step processes its logits in place (see decode).
        ``stop`` (sampling.check_stop_args' dict, or None): per-row stopping in the bookkeeping launch of the selection (DESIGN.md
        "Per-row stopping"); armed with ``eos_token`` (the pad id, the first eos id) on the prefill / extend call and passed
        again to every cached step; not with ``beam``.
        ``logprobs`` (None = off, or n_top in [0, 20]): one launch between the selection and its bookkeeping writes the selected
        token's log-probability under the RAW distribution of the step, and the n_top most probable tokens, into column
        step of the cache's lp / top_id / top_lp buffers (DESIGN.md "Token log-probabilities"); passed like ``stop``; not with
        ``beam``.
        ``constraint`` (a list of one sampling.TokenTrie per row, or None): the trie constraint in the
        processors' launch (DESIGN.md "Constrained decoding") -- it counts as a processor: the first token comes from a processed
        copy, with ``logprobs`` the step works on the second buffer; passed like ``processors``; not with ``beam``.
        ``guidance`` ((guidance_scale, guidance_min_p), or None): classifier-free guidance (DESIGN.md
        "Classifier-free guidance").  The batch is 2R ragged rows: rows [0, R) the prompts, rows [R, 2R) the negative prompts.  One
        launch combines row r with row R + r in front of the processors, everything from there to the bookkeeping runs over the
        first R rows (and the first R rows of the per-row buffers), one launch copies the token to row R + r and advances its
        position.  It counts as a processor (first token from a copy; with ``logprobs`` the second buffer, the log-probabilities
        are those of the raw conditional rows); passed like ``processors``; not with ``beam``, not when continuing a cache.
        ``lengths`` (int [B], 1 <= len_b <= S; prefill with use_cache=True only): the rows of ``inputs_embeds`` are prompts
        of different lengths, right-padded to S.  Row b's logits are those of its position len_b - 1, and the cache keeps one
        write position per row (len_b, then + 1 per step) -- see DESIGN.md, "Ragged batches"."""
        extending = past_key_values is not None and inputs_embeds is not None
        if plan is None:
            plan = self.selection_plan(sampling=sampling, beam=beam, processors=processors, stop=stop, logprobs=logprobs,
                                       constraint=constraint, guidance=guidance, vocab=self.V)
        if plan.guidance is not None and extending:
            raise NotImplementedError("guidance does not continue from a KV cache")
        if plan.is_contrast and extending:
            raise NotImplementedError("contrastive search does not continue from a KV cache")
        if lengths is not None and (labels is not None or (past_key_values is not None and not extending) or not use_cache):
            raise ValueError("lengths= applies to the prefill call and to inputs_embeds appended to a cache (use_cache=True, no "
                             "labels); a ragged cache keeps its per-row positions for the steps that follow")
        if labels is not None:
            if inputs_embeds is None:
                inputs_embeds = self.embed_ids(input_ids)
            return self.forward_loss(inputs_embeds, labels, output_hidden_states, return_logits)
        if extending:
            # inputs_embeds appended to a cache (the HF GPT-Neo forward takes this pair; positions follow the past): one chunk pass
            if input_ids is not None:
                raise ValueError("pass input_ids or inputs_embeds, not both")
            if plan.is_beam:
                raise NotImplementedError("beam search does not continue from a KV cache")
            logits, cache, full = self.extend(past_key_values, inputs_embeds, lengths=lengths, cache_hint=cache_hint)
            out = LMOutput(logits=logits.unsqueeze(1), past_key_values=cache, hidden_states=None, loss=None, full_logits=full)
            if eos_token is not None:
                self._arm_first_token(out, logits, cache, eos_token, seed, plan)
            return out
        if past_key_values is not None:
            if not feed_back and input_ids is None:
                raise ValueError("cached decoding takes input_ids (reference sampling.py:88-90)")
            if not feed_back and input_ids.shape[1] != 1:
                # several new tokens against the cache (the reference LM takes any input_ids length with past_key_values; its
                # generate() only ever sends one, sampling.py:86-90): the causal mask makes this exactly T single-token steps in
                # order, each appending its K / V -- run as such, logits (B, T, V) stacked
                T = input_ids.shape[1]
                if T == 0:
                    raise ValueError("cached decoding needs at least one new token")
                rows = []
                for i in range(T):      # only the LAST position selects a token (history / RNG step / eos latch untouched before)
                    lg, tok = self.decode(input_ids[:, i:i + 1], past_key_values, select=i == T - 1, plan=plan)
                    rows.append(lg.clone())
                return LMOutput(logits=torch.stack(rows, 1), past_key_values=past_key_values, next_token=tok, loss=None,
                                eos_state=past_key_values.sample_state)
            logits, tok = self.decode(None if feed_back else input_ids, past_key_values, plan=plan)
            return LMOutput(logits=logits.unsqueeze(1), past_key_values=past_key_values, next_token=tok, loss=None,
                            eos_state=past_key_values.sample_state)
        if inputs_embeds is None:
            inputs_embeds = self.embed_ids(input_ids)
        if use_cache:
            logits, cache, hs = self.prefill(inputs_embeds, cache_hint, output_hidden_states, reuse_cache, lengths=lengths,
                                             keep_x=plan.is_contrast and eos_token is not None)
            # generate() only reads the last position, so only that row is computed
            out = LMOutput(logits=logits.unsqueeze(1), past_key_values=cache, hidden_states=hs, loss=None)
            if eos_token is not None:
                self._arm_first_token(out, logits, cache, eos_token, seed, plan)
            return out
        x, hs = self._blocks_prefill(inputs_embeds, None, output_hidden_states)
        B, S, _ = inputs_embeds.shape
        logits = self._full_logits(x, B * S).view(B, S, self.V)
        return LMOutput(logits=logits, past_key_values=None, hidden_states=hs, loss=None)

    def embed_ids(self, ids: torch.Tensor) -> torch.Tensor:
        ids = ids.to(self.device).contiguous()
        out = torch.empty(ids.shape[0], ids.shape[1], self.d, dtype=BF16, device=self.device)
        return ops.embedding(ids, self.wte, out)

    # -------------------------------------------------------------- prefill
    def _blocks_prefill(self, embeds: torch.Tensor, cache: Optional[KVCache], want_hidden=False, lse_out=None, chunk=False,
                        tree=None, key_scale=None):
        """The blocks over B x S new rows.  ``chunk``: the rows continue ``cache`` -- row b's S rows sit at cache.d_pos[b * pos_stride]
        + s, their K / V are appended there and they attend over the cached keys (mg_attn_prefill_cached_bf16); every GEMM, adapter and
        epilogue launch is the prefill's.  ``tree`` (with ``chunk``; tree_forward): the rows are trie nodes -- (d_pos int32 [B], off,
        sub int32 [B, S], p_min) -- row s goes to slot d_pos[b] + s at position d_pos[b] + off[b, s] and sees the cache below d_pos[b]
        and the chunk rows j <= s < sub[b, j] (mg_rotary_split_at_bf16 / mg_attn_prefill_tree_bf16 in place of the chunk's two).  ``key_scale``
        (check_key_scale; the plain cache-less bf16 branch only): fp32 [B, S], every block and head multiplies the score of key j of
        row b by key_scale[b, j] before the causal mask (mg_attn_prefill_scaled_bf16 in place of mg_attn_prefill_bf16)."""
        B, S, d = embeds.shape
        assert d == self.d
        self._current_packs()
        if key_scale is not None:
            mode = ("a tree forward" if tree is not None else "a chunk that continues a KV cache" if chunk
                    else "the fp8 attention mode" if self.fp8_mode and self.fp8_attn and cache is None else None)
            if mode is not None:
                raise NotImplementedError(f"key_scale is not implemented for {mode}")
            if key_scale.dtype != torch.float32 or tuple(key_scale.shape) != (B, S) or key_scale.device != embeds.device:
                raise ValueError(f"key_scale must be fp32 ({B}, {S}) on {embeds.device}, got {key_scale.dtype} {tuple(key_scale.shape)}")
        if S > self.cfg.max_position_embeddings:
            raise ValueError(f"sequence length {S} exceeds max_position_embeddings")
        dev = self.device
        x = embeds.to(BF16).contiguous().view(B * S, d)
        M = B * S
        vt_ld = ops.ceil_to(S, 32)
        q = torch.empty(B, self.H, S, 256, dtype=BF16, device=dev)
        vt = None if chunk else torch.empty(B, self.H, vt_ld // 32, 256, 32, dtype=BF16, device=dev)   # V^T in 32-key tiles
        if cache is None:   # no cache requested: one scratch K/V shared by all layers
            kscr = torch.empty(B, self.H, S, 256, dtype=BF16, device=dev)
            vscr = torch.empty(B, self.H, S, 256, dtype=BF16, device=dev)
        # MAGMA_v1 blocks (mlp adapter of the 'normal' type): out_proj and the adapter's up-projection are ONE GEMM over the
        # concatenated input [ctx | t] against [W_out | W_up] -- x' = that + b_up + m + x, the sum the reference forms (reference
        # adapters.py:38-39 + the block's residual) in another association order.  One launch, one epilogue and one (M, d)
        # round trip (the attention output `a`) less per block; at M = 456 also one split-K fix-up less.  MAGMA_PREFILL_CAT=0: off.
        r_cat = 0
        if self.cat_up and not self.fp8_mode:
            r_cat = max([ly.mlp_adapter[0].N for ly in self.layers if self._ensure_out_up(ly) is not None] + [0])
        ctx_t = torch.empty(M, d + r_cat, dtype=BF16, device=dev)
        ctx = ctx_t[:, :d]
        hs = [x.view(B, S, d)] if want_hidden else None
        for li, ly in enumerate(self.layers):
            ln = ops.layernorm(x, ly.ln_g, ly.ln_b, self.eps)
            lnq = self._quantize(ln) if self.fp8_mode else None             # shared by qkv (and fc_in in "all" mode)
            h_fused = None
            if self.fuse_in and not self.fp8_mode:
                # qkv and gelu(fc_in) in ONE launch over [q | k | v | fc_in] (gelu_new on the fc_in columns only).  At the
                # BASELINE prefill (M = 8 x 57 = 456 rows) the 256x256 kernel then covers the 28 672 columns with
                # 2 x 112 = 224 tiles -- one round of the 256 CUs, no split-K fix-up -- instead of 384 + 512 tiles of 128^2
                # in two under-filled launches
                d3 = 3 * self.d
                qh = ops.gemm(ln, ly.in_cat, act=ops.MG_ACT_GELU_NEW, act_n0=d3, tile=256 if 256 < M <= 512 else 0)
                qkv, h_fused = qh[:, :d3], qh[:, d3:]
            else:
                qkv = self._linear(ly, "qkv", ly.qkv, ln, lnq)
            kc, vc = (cache.k[li], cache.v[li]) if cache is not None else (kscr, vscr)
            if tree is not None:
                t_pos, t_off, t_sub, t_pmin = tree
                ops.rotary_split_at(qkv, B, S, self.H, self.rot, self.sin_t, self.cos_t, q, kc, vc, t_pos, t_off)
                ops.attn_prefill_tree(q, kc, vc, ctx, B, self.H, S, t_pos, t_sub, p_min=t_pmin, pos_stride=1)
            elif chunk:
                ops.rotary_split(qkv, B, S, self.H, self.rot, self.sin_t, self.cos_t, q, kc, vc, d_pos=cache.d_pos,
                                 pos_stride=cache.pos_stride)
                ops.attn_prefill_cached(q, kc, vc, ctx, B, self.H, S, cache.d_pos, pos_stride=cache.pos_stride)
            elif self.fp8_mode and self.fp8_attn and cache is None and qkv.is_contiguous():
                # BASELINE config[4]: the attention core on the fp8 MFMA as well (no KV cache to fill: cached decoding reads bf16)
                a8 = ops.rotary_split_fp8(qkv, B, S, self.H, self.rot, self.sin_t, self.cos_t)
                ops.attn_prefill_fp8(a8, ctx, lse=None if lse_out is None else lse_out[li])
            else:
                ops.rotary_split(qkv, B, S, self.H, self.rot, self.sin_t, self.cos_t, q, kc, vc, pos0=0, vt=vt)
                if key_scale is not None:
                    ops.attn_prefill_scaled(q, kc, vt, ctx, B, self.H, S, key_scale, lse=None if lse_out is None else lse_out[li])
                else:
                    ops.attn_prefill(q, kc, vt, ctx, B, self.H, S, lse=None if lse_out is None else lse_out[li])
            if r_cat and ly.out_up is not None and ly.mlp_adapter[0].N == r_cat:
                h = h_fused if h_fused is not None else self._linear(ly, "fc_in", ly.fc_in, ln, lnq, act=ops.MG_ACT_GELU_NEW)
                m = ops.gemm(h, ly.fc_out)
                ops.gemm(m, ly.mlp_adapter[0], out=ctx_t[:, d:], act=ops.MG_ACT_RELU)
                x = ops.gemm(ctx_t, ly.out_up, residuals=(m, x))
                if want_hidden:
                    hs.append(x.view(B, S, d))
                continue
            # x @ w^T under the projection's fp8 name; a parallel adapter reads ln_1's output, its up-projection stays on ops.gemm
            L = lambda name: lambda t, w, **kw: self._linear(ly, name, w, t, **kw)  # noqa: E731
            a = self._linear(ly, "out", ly.out, ctx)
            if ly.attn_adapter is not None:
                par = ly.attn_par
                a = self._adapter(L("attn_dn"), ops.gemm if par is not None else L("attn_up"), ly.attn_adapter, ly.attn_act,
                                  ly.attn_ad_ln, ln if par is not None else a, par, (a,))
            h = h_fused if h_fused is not None else self._linear(ly, "fc_in", ly.fc_in, ln, lnq, act=ops.MG_ACT_GELU_NEW)
            if ly.mlp_adapter is not None:
                par = ly.mlp_par
                m = self._linear(ly, "fc_out", ly.fc_out, h)
                x = self._adapter(L("mlp_dn"), ops.gemm if par is not None else L("mlp_up"), ly.mlp_adapter, ly.mlp_act,
                                  ly.mlp_ad_ln, ln if par is not None else m, par, (m, a, x))
            else:
                x = self._linear(ly, "fc_out", ly.fc_out, h, residuals=(a, x))
            if want_hidden:
                hs.append(x.view(B, S, d))
        return x, hs

    @staticmethod
    def check_lengths(lengths, B: int, S: int) -> torch.Tensor:
        """Prompt lengths of a right-padded batch as a host int64 [B] tensor; 1 <= len_b <= S."""
        lens = torch.as_tensor(lengths).detach().to("cpu")
        if lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
            raise TypeError(f"lengths must be integers, got {lens.dtype}")
        lens = lens.to(torch.int64)
        if lens.ndim != 1 or lens.shape[0] != B:
            raise ValueError(f"lengths must have shape ({B},) (one length per row), got {tuple(lens.shape)}")
        if int(lens.min()) < 1 or int(lens.max()) > S:
            raise ValueError(f"every length must lie in [1, {S}] (the padded sequence length), got {lens.tolist()}")
        return lens

    def prefill(self, embeds: torch.Tensor, cache_hint: Optional[int] = None, want_hidden=False,
                reuse_cache: bool = False, lengths=None, keep_x: bool = False):
        """``keep_x``: the last block's output for every prompt row stays on the cache (cache.prefill_x, (B, S, d)) until
        _arm_contrast has turned it into the context store."""
        B, S, _ = embeds.shape
        ragged = lengths is not None
        if ragged:
            lens = self.check_lengths(lengths, B, S)
        n_pos = self.cfg.max_position_embeddings
        Smax = min(n_pos, ops.ceil_to(S + (cache_hint if cache_hint else 256), 64))
        if reuse_cache:
            # generate() owns the cache for the duration of one call: keep one KV cache (and the
            # hipGraph of the token step captured on it) per shape instead of re-allocating and
            # re-capturing for every call.  Ragged and uniform caches never share an entry: the
            # position layout (and with it the captured launches) differ
            key = (B, Smax, ragged)
            cache = self._cache_pool.pop(key, None)
            pooled = self._cache_pool_max > 0                            # a bound of 0: nothing is kept
            while pooled and len(self._cache_pool) >= self._cache_pool_max:      # least recently used shape goes first
                self._cache_pool.pop(next(iter(self._cache_pool)))
            if cache is None:
                cache = KVCache(self.L, B, self.H, Smax, self.device, ragged=ragged)
            if pooled:
                self._cache_pool[key] = cache                            # (re-)insert as most recently used
        else:
            cache = KVCache(self.L, B, self.H, Smax, self.device, ragged=ragged)
        # right padding: the prefill is unchanged -- under the causal mask a valid row attends to valid keys only, and the
        # K / V the padded rows leave in slots >= len_b are overwritten by decode steps before any row reads them
        x, hs = self._blocks_prefill(embeds, cache, want_hidden)
        cache.owner = weakref.ref(self)
        cache.prefill_x = x.view(B, S, self.d) if keep_x else None
        cache._rows, cache.pending = (lens.clone() if ragged else None), None
        if ragged:
            cache.pos = int(lens.max())
            cache._rows_at = cache.pos
            cache.d_pos.copy_(lens.to(torch.int32), non_blocking=True)       # no stream sync (as sample_state in forward)
            rows = (torch.arange(B, dtype=torch.int64) * S + lens - 1).to(self.device, non_blocking=True)
            last = x.index_select(0, rows)                       # row len_b - 1 of every sequence
        else:
            cache.pos = S
            cache.d_pos.fill_(S)
            last = x.view(B, S, self.d)[:, S - 1, :]             # strided rows, no copy
        xl = ops.layernorm(last, self.lnf_g, self.lnf_b, self.eps)
        logits = self._head(xl)
        return logits, cache, hs

    def detach_cache(self, cache: KVCache) -> KVCache:
        """Take ``cache`` out of the reuse pool: no later generate() call overwrites it."""
        for key, c in list(self._cache_pool.items()):
            if c is cache:
                del self._cache_pool[key]
        return cache

    def extend(self, cache: KVCache, embeds: torch.Tensor, lengths=None, cache_hint: Optional[int] = None):
        """Append B x T new rows (``lengths``: T_b >= 1 of them per row, right-padded) to ``cache`` and run the blocks over them
        only: row b's rows take positions p_b .. p_b + T_b - 1 (p_b = its write position; a token a generate() call left
        pending -- selected, not fed back -- goes first).  Grows the cache when p_b + T_b + cache_hint exceeds Smax.  Returns
        (fp32 logits (B, V) of every row's last new position, the cache -- positions advanced by T_b --, the (B, T', V) logits
        of the caller's T rows as a lazy value -- a pending token's own logits are not among them)."""
        if not isinstance(cache, KVCache):
            raise TypeError(f"past_key_values must be this engine's KVCache, got {type(cache).__name__}")
        if cache.beam is not None and cache.beam.k > 1:
            raise NotImplementedError("a beam-search cache cannot be continued")
        if embeds.ndim != 3 or embeds.shape[0] != cache.B or embeds.shape[2] != self.d:
            raise ValueError(f"inputs_embeds must be ({cache.B}, T, {self.d}) for this cache, got {tuple(embeds.shape)}")
        B, T, _ = embeds.shape
        if T < 1:
            raise ValueError("continuing a cache needs at least one new position per row")
        lens = self.check_lengths(lengths, B, T) if lengths is not None else None
        T_in, shift = T, None
        if cache.pending is not None and bool((cache.pending >= 0).any()):
            has = cache.pending >= 0
            if lens is None:
                lens = torch.full((B,), T, dtype=torch.int64)
            idx = has.nonzero().squeeze(1).to(self.device)
            e = torch.zeros(B, T + 1, self.d, dtype=BF16, device=self.device)
            e[:, :T] = embeds
            e[idx, 1:] = embeds.to(BF16).index_select(0, idx)
            e[idx, :1] = self.embed_ids(cache.pending.clamp(min=0).view(B, 1).to(self.device)).index_select(0, idx)
            embeds, lens, T = e, lens + has.to(torch.int64), T + 1
            shift = has.to(torch.int64)
        rows = cache.rows_pos()
        add = lens if lens is not None else torch.full((B,), T, dtype=torch.int64)
        n_pos = self.cfg.max_position_embeddings
        end = rows + add
        if int(end.max()) > n_pos:
            raise ValueError(f"continuing the cache reaches position {int(end.max())}, beyond max_position_embeddings = {n_pos}")
        cache.pending = None
        need = max(int(end.max()), int(rows.max()) + T) + (cache_hint or 0)
        self.detach_cache(cache)
        if need > cache.Smax:
            cache.grow(min(n_pos, ops.ceil_to(need, 64)))
        if lens is not None and not cache.ragged:
            cache.set_rows(rows)
        x, _ = self._blocks_prefill(embeds, cache, chunk=True)
        if cache.ragged:
            cache.d_pos.add_(add.to(torch.int32).to(self.device, non_blocking=True))
            cache._rows, cache.pos = end, int(end.max())
            cache._rows_at = cache.pos
        else:
            cache.d_pos.add_(T)
            cache.pos += T
        if lens is not None:
            last = x.index_select(0, (torch.arange(B, dtype=torch.int64) * T + lens - 1).to(self.device, non_blocking=True))
        else:
            last = x.view(B, T, self.d)[:, T - 1, :]
        logits = self._head(ops.layernorm(last, self.lnf_g, self.lnf_b, self.eps))
        if shift is None:
            full = LMOutput.lazy(lambda: self._full_logits(x, B * T).view(B, T, self.V))
        else:       # the caller's rows only: row b's input t sits at combined row t + 1 when a pending token went first
            rows = (torch.arange(B)[:, None] * T + torch.arange(T_in)[None, :] + shift[:, None]).reshape(-1).to(self.device)
            full = LMOutput.lazy(lambda: self._full_logits(x.index_select(0, rows), B * T_in).view(B, T_in, self.V))
        return logits, cache, full

    def tree_forward(self, cache: KVCache, rows) -> torch.Tensor:
        """The blocks over a TREE of new rows against ``cache`` (Magma.rank; DESIGN.md "Ranking choices"): ``rows`` = (token, off, sub)
        int32 (B, T) host or device tensors as sampling.pad_trie_rows lays them out -- the trie's non-root nodes in depth-first
        preorder, right-padded.  Node t of row b is fed wte[token[b, t]] at position p_b + off[b, t] (p_b = the row's write
        position), its K / V go to the scratch slot p_b + t, and it attends to the cached keys below p_b and to the nodes
        j <= t < sub[b, j] (itself and its ancestors).  _blocks_prefill in its third chunk mode: every GEMM, adapter and epilogue
        launch is the prefill's.  The cache's positions are NOT advanced and nothing below p_b is written: the cache stays what
        it was (slots >= p_b are scratch, as for any cache), so one prompt cache serves any number of trees.  Returns the
        final hidden rows (B * T, d); the caller runs ln_f and the head on the rows it needs."""
        if not isinstance(cache, KVCache):
            raise TypeError(f"tree_forward needs this engine's KVCache, got {type(cache).__name__}")
        token, off, sub = (torch.as_tensor(t) for t in rows)
        if token.ndim != 2 or token.shape[0] != cache.B or off.shape != token.shape or sub.shape != token.shape:
            raise ValueError(f"rows must be three ({cache.B}, T) tensors, got {tuple(token.shape)}, {tuple(off.shape)}, {tuple(sub.shape)}")
        B, T = token.shape
        pos = cache.rows_pos()
        if cache.pending is not None and bool((cache.pending >= 0).any()):
            raise ValueError("tree_forward: the cache holds a token that has not been fed back; continue it first")
        if int(pos.min()) < 1:
            raise ValueError("tree_forward needs at least one cached position in front of every tree")
        n_pos = self.cfg.max_position_embeddings
        if int(pos.max()) + T > n_pos:
            raise ValueError(f"the tree's {T} rows behind position {int(pos.max())} exceed max_position_embeddings = {n_pos}")
        if int(pos.max()) + T > cache.Smax:
            self.detach_cache(cache)
            cache.grow(min(n_pos, ops.ceil_to(int(pos.max()) + T, 64)))
        dev = self.device
        d_pos = cache.d_pos if cache.ragged else cache.d_pos[:1].expand(B).contiguous()
        to32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()  # noqa: E731
        embeds = self.embed_ids(token.to(torch.int64))
        x, _ = self._blocks_prefill(embeds, cache, chunk=True, tree=(d_pos, to32(off), to32(sub), int(pos.min())))
        return x

    HEAD_SLAB = 1024          # rows of fp32 logits alive at once in head_token_logprobs (x Vp x 4 bytes: 0.2 GB at V = 50400)

    def head_token_logprobs(self, x: torch.Tensor, rows: torch.Tensor, row_of: torch.Tensor, token: torch.Tensor) -> torch.Tensor:
        """ln_f and the fp32 head on the hidden rows ``x[rows]`` (``rows`` int64 [R], host), HEAD_SLAB rows at a time, and per entry
        i the log-probability of ``token[i]`` under logits row ``row_of[i]`` of those R (both int32 [N], host, ``row_of``
        ascending): mg_token_logprobs_rows_f32, no logits row is copied for a node's fan-out.  Returns fp32 [N] on the device."""
        N, R = row_of.numel(), rows.numel()
        lp = torch.empty(N, dtype=torch.float32, device=self.device)
        if N == 0:
            return lp
        assert bool((row_of[1:] >= row_of[:-1]).all()) and int(row_of[0]) >= 0 and int(row_of[-1]) < R
        rows_d, tok_d = rows.to(self.device), token.to(self.device)
        edge = torch.searchsorted(row_of, torch.arange(0, R + self.HEAD_SLAB, self.HEAD_SLAB, dtype=row_of.dtype)).tolist()
        logits = torch.empty(min(R, self.HEAD_SLAB), self.Vp, dtype=torch.float32, device=self.device)
        for k, r0 in enumerate(range(0, R, self.HEAD_SLAB)):
            e0, e1 = edge[k], edge[k + 1]
            if e1 == e0:
                continue
            n = min(self.HEAD_SLAB, R - r0)
            xl = ops.layernorm(x.index_select(0, rows_d[r0:r0 + n]), self.lnf_g, self.lnf_b, self.eps)
            # score's head (_target_logits): the tile GEMM whatever n is -- a row's logits do not depend on how many rows share the
            # launch (_head would switch to the weight-streaming kernel at n <= 16), so a choice keeps its bits from group to group
            ops.gemm(xl, self.head, out=logits[:n])
            ops.token_logprobs_rows(logits[:n, : self.V], (row_of[e0:e1] - r0).to(self.device), tok_d[e0:e1], lp[e0:e1])
        return lp

    def _head(self, xl: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        M = xl.shape[0]
        if out is None:
            out = torch.empty(M, self.Vp, dtype=torch.float32, device=self.device)
        if M <= 16:
            ops.gemm_skinny(xl, self.head, out=out)
        else:
            ops.gemm(xl, self.head, out=out)
        return out[:, : self.V]

    def _full_logits(self, x: torch.Tensor, M: int) -> torch.Tensor:
        xl = ops.layernorm(x, self.lnf_g, self.lnf_b, self.eps)
        out = torch.empty(M, self.Vp, dtype=BF16, device=self.device)
        ops.gemm(xl, self.head, out=out)
        return out[:, : self.V]

    # --------------------------------------------------------------- decode
    def _alloc_decode_state(self, cache: KVCache, rows: Optional[int] = None):
        """``rows``: the rows of the step when they are not the cache's (a speculative step: B * T)."""
        B, d, dev = rows or cache.B, self.d, self.device
        ff = self.layers[0].fc_in.N
        st = _Layer()
        e = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
        st.ids = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        st.xa, st.xb = e(B, d), e(B, d)
        st.ln, st.qkv = e(B, d), e(B, 3 * d)
        st.ctx, st.a, st.a2, st.h, st.m = e(B, d), e(B, d), e(B, d), e(B, ff), e(B, d)
        r_mlp = max([ly.mlp_adapter[0].N for ly in self.layers if ly.mlp_adapter] + [8])
        r_att = max([ly.attn_adapter[0].N for ly in self.layers if ly.attn_adapter] + [8])
        st.t, st.ta = e(B, r_mlp), e(B, r_att)
        st.tcat = e(B, r_mlp + r_att)      # [mlp bottleneck | attention bottleneck] side by side (fused up-projection)
        st.ctx_t = e(B, d + r_mlp)         # [attention context | mlp bottleneck]: input of the [W_out | W_up] GEMV (fold_dn)
        st.lnf = e(B, d)
        st.ad_ln = e(B, d)                 # LayerNorm output in front of an adapter built with add_layernorm
        st.logits = e(B, self.Vp, dt=torch.float32)
        st.logits_proc = None      # with logprobs AND processors: the copy the processors and the selection work on (SelectionPlan.arm)
        st.token = torch.zeros(B, dtype=torch.int64, device=dev)
        st.graphs = {}             # StepKey (SelectionPlan.graph_key) -> captured hipGraph
        st.steps = 0
        st.colaunch = True
        st.rows, st.T = B, 1       # T > 1: the rows are T consecutive positions of each of the cache's sequences (_ensure_spec_state)
        # shared session prefix: the partials every block's prefix launch leaves for its attention launch (one buffer: the launches
        # of a step are ordered), (prefix_P, buffer) as the attention launches take it
        st.shared = (cache.prefix_P, ops.prefix_part(B, self.H, cache.prefix_P, dev)) if cache.prefix_P else None
        return st

    def _decode_step(self, cache: KVCache, st, plan: SelectionPlan, feed_back: bool = False):
        """Enqueue one token step for all B sequences (graph-capturable: no
        allocation, no sync, position read from cache.d_pos on the device): embedding, per layer the launch sequence of the
        kind planned for it (st.kinds, _ensure_decode_state), the head, token selection under ``plan``.
        ``feed_back``: the input ids are the tokens the previous step selected (st.token, still on the device) -- the
        reference's loop feeds exactly those back (sampling.py:88-90) -- instead of ids copied in from the caller."""
        x = self._step_logits(cache, st, st.token.view(cache.B, 1) if feed_back else st.ids)
        if plan.is_contrast and plan.select:
            self._select_contrast(x, cache, st, plan)
        elif not plan.select:
            ops.advance_pos(cache.d_pos, pos_stride=cache.pos_stride)   # teacher-forced position: nothing selected, nothing recorded
        elif plan.second_buffer:
            # the processors run in place: they and the selection get a copy (one device copy inside the step), the
            # log-probabilities read the untouched st.logits
            st.logits_proc.copy_(st.logits)
            self.select_token(st.logits_proc[:, : self.V], cache, plan, out=st.token, advance=True, raw=st.logits[:, : self.V])
        else:
            self.select_token(st.logits[:, : self.V], cache, plan, out=st.token, advance=True)


    def _step_logits(self, cache: KVCache, st, ids):
        """The step up to its logits (st.logits) for the st.rows rows whose token ids are ``ids`` (rows, 1): embedding, the blocks,
        the head.  Returns the last block's output."""
        B = st.rows
        ops.embedding(ids, self.wte, st.xa.view(B, 1, self.d))
        x, xn = st.xa, st.xb
        for li, (ly, kind) in enumerate(zip(self.layers, st.kinds)):
            getattr(self, "_block_" + kind)(cache, st, li, ly, ly.w8 if st.w8 else ly.w4 if st.w4 else ly, x, xn)
            x, xn = xn, x
        if B > 16:
            ops.layernorm(x, self.lnf_g, self.lnf_b, self.eps, out=st.lnf)
            ops.gemm(st.lnf, self.head, out=st.logits)
        else:
            head = self.head_w8 if st.w8 else self.head_w4 if st.w4 else self.head_dec
            ops.gemm_skinny(x, head, out=st.logits, ln_fold=(head.colsum, self.d, self.eps))
        return x

    def _spec_step(self, cache: KVCache, st, plan: SelectionPlan):
        """Enqueue one speculative step (graph-capturable): the B * T rows st.ids -- per sequence its last emitted token and its
        drafts -- through the blocks against the cache of B rows (chunk attention: row t of a sequence attends up to its own
        position), the selection of every row -- its argmax, or under a sampled plan (plan.spec_rows) the chunk selection: fed row
        b * T + t under sequence b's record at the counter count[b] + t, the rows the bookkeeping never reads skipped --, and the
        bookkeeping launch that accepts, records, advances and drafts again (with stop sequences: mg_spec_finish_seq)."""
        B, T = cache.B, st.T
        self._step_logits(cache, st, st.ids)
        if plan.spec_rows is None:
            ops.argmax(st.logits[:, : self.V], out=st.token)
        else:
            ops.sample_chunk(st.logits[:, : self.V], T, st.sample_rows, st.count, cache.finish, n_draft=st.n_draft,
                             history_cols=cache.history.shape[1], warp=plan.spec_rows, out=st.token)
        ops.spec_finish(st.ids.view(B, T), st.n_draft, st.token, cache.history, st.count, cache.finish, cache.stop_table,
                        len(plan.stop[0]), st.limit, st.lookup, st.lookup_len, st.stats, cache.sample_state, T - 1, plan.mode[2],
                        self.V, cache.d_pos, **(dict(n_seq=len(plan.stop[1])) if plan.stop[1] else {}))

    # One method per block kind (_block_kind): x -> xn for layer li.  ``src`` holds the block's weight-streaming operands: the
    # layer itself, or its e4m3 / MXFP4 copies (ly.w8 / ly.w4) under W8A16 / W4A16 -- the same launches.  On a ragged cache (pos_stride 1) every
    # attention launch reads row b's position d_pos[b].
    def _dec_in(self, st, src, x):
        # ln_1 + qkv + fc_in(+gelu) in ONE weight-streaming launch
        ops.gemm_skinny(x, src.dec_in, out=st.qkv, ln_fold=(src.dec_in.colsum, self.d, self.eps),
                        split=(3 * self.d, st.h, ops.MG_ACT_GELU_NEW, src.dec_in.bias_b), variant=self._dec_in_variant)

    def _attn_prefix(self, cache, st, li):
        # shared session prefix, kernel 1: every row's partial attention over the one prefix, for the attention launch that follows
        ops.attn_decode_prefix(st.qkv, cache.prefix_k[li, 0], cache.prefix_v[li, 0], st.shared[1], cache.B, self.H, cache.prefix_P,
                               cache.d_pos, self.rot, self.sin_t, self.cos_t, pos_stride=cache.pos_stride)

    def _attn_gemv(self, cache, st, li, ctx, gemv):
        # attention workgroups + one GEMV's workgroups in one grid (they are independent branches of the parallel block; the
        # latency-bound attention hides under the weight stream)
        if st.shared is not None:
            self._attn_prefix(cache, st, li)
            ops.decode_attn_gemv(st.qkv, cache.k[li], cache.v[li], ctx, cache.B, self.H, cache.d_pos, self.rot, self.sin_t,
                                 self.cos_t, gemv, pos_stride=cache.pos_stride, shared=st.shared)
            return
        if st.T > 1 and not st.colaunch:      # MAGMA_SPEC_COLAUNCH=0: the chunk attention alone, then the GEMV alone (two launches)
            ops.attn_decode_chunk(st.qkv, cache.k[li], cache.v[li], ctx, cache.B, st.T, self.H, cache.d_pos, self.rot, self.sin_t,
                                  self.cos_t, pos_stride=cache.pos_stride)
            ops.gemm_skinny(gemv[0], gemv[1], out=gemv[2], **gemv[3])
            return
        if st.T > 1:      # a speculative step: T consecutive positions per sequence, the GEMV over all B * T rows
            ops.decode_attn_gemv(st.qkv, cache.k[li], cache.v[li], ctx, cache.B, self.H, cache.d_pos, self.rot, self.sin_t,
                                 self.cos_t, gemv, pos_stride=cache.pos_stride, chunk=st.T)
            return
        ops.decode_attn_gemv(st.qkv, cache.k[li], cache.v[li], ctx, cache.B, self.H, cache.d_pos, self.rot, self.sin_t, self.cos_t,
                             gemv, pos_stride=cache.pos_stride)

    def _block_fold2(self, cache, st, li, ly, src, x, xn):
        # MAGMA_DECODE_FOLD=2: attention || fc_out (context row lands in st.ctx_t), adapter-down alone, [W_out | W_up] GEMV
        r = ly.mlp_adapter[0].N
        ctx, t = st.ctx_t[:, : self.d], st.ctx_t[:, self.d: self.d + r]
        self._dec_in(st, ly, x)
        self._attn_gemv(cache, st, li, ctx, (st.h, ly.fc_out, st.m, {}))
        ops.gemm_skinny(st.m, ly.mlp_adapter[0], out=t, act=ops.MG_ACT_RELU, variant=self._dec_dn_variant)
        ops.gemm_skinny(st.ctx_t[:, : self.d + r], ly.out_up, out=xn, residuals=(st.m, x), variant=self._dec_cat_variant)

    def _block_fold1(self, cache, st, li, ly, src, x, xn):
        # three launches (fold_dn).  launch 2: attention || [fc_out ; W_dn W_fc_out]: m and the adapter bottleneck t
        # from ONE pass over h; the context row lands beside t in st.ctx_t.  launch 3: x' = [W_out | W_up] [ctx ; t] + b_up + m + x
        r = ly.mlp_adapter[0].N
        ctx, t = st.ctx_t[:, : self.d], st.ctx_t[:, self.d: self.d + r]
        self._dec_in(st, ly, x)
        self._attn_gemv(cache, st, li, ctx, (st.h, ly.fc_dn, st.m, {"split": (self.d, t, ops.MG_ACT_RELU, ly.fc_dn.bias_b)}))
        ops.gemm_skinny(st.ctx_t[:, : self.d + r], ly.out_up, out=xn, residuals=(st.m, x))

    def _block_grouped(self, cache, st, li, ly, src, x, xn):
        # four launches: [ln_1+qkv+fc_in] -> [attention || fc_out] -> [out_proj || adapter-down] -> [adapter-up + the block's
        # three residuals]
        t = st.t[:, : ly.mlp_adapter[0].N]
        self._dec_in(st, src, x)
        self._attn_gemv(cache, st, li, st.ctx, (st.h, src.fc_out, st.m, {}))
        ops.gemm_skinny2((st.ctx, src.out, st.a, {}), (st.m, src.mlp_adapter[0], t, {"act": ly.mlp_act}))
        ops.gemm_skinny(t, src.mlp_adapter[1], out=xn, residuals=(st.m, st.a, x))

    def _block_v2(self, cache, st, li, ly, src, x, xn):
        # MAGMA_v2 (attention AND mlp adapters): 5 launches.  x' = up_m(t) + up_a(ta) + m + a + x is ONE GEMV over
        # the concatenated bottlenecks [t | ta] against [W_up_m | W_up_a] (the adapter outputs only ever appear summed)
        r1 = ly.mlp_adapter[0].N
        t, ta = st.tcat[:, :r1], st.tcat[:, r1: r1 + ly.attn_adapter[0].N]
        self._dec_in(st, src, x)
        self._attn_gemv(cache, st, li, st.ctx, (st.h, src.fc_out, st.m, {}))
        ops.gemm_skinny2((st.ctx, src.out, st.a, {}), (st.m, src.mlp_adapter[0], t, {"act": ly.mlp_act}))
        ops.gemm_skinny(st.a, src.attn_adapter[0], out=ta, act=ly.attn_act)
        ops.gemm_skinny(st.tcat[:, : src.up_cat.Kp], src.up_cat, out=xn, residuals=(st.m, st.a, x))

    def _block_generic(self, cache, st, li, ly, src, x, xn, wide=False):
        # every other block (no MLP adapter, parallel adapters, adapters with a LayerNorm or erf-GELU): attention alone, then
        # out_proj and fc_out from src -- e4m3 under W8A16 --, the small adapter projections in bf16 (_adapter).  ``wide``:
        # called from _block_wide, which has made ln_1, qkv and h
        G = ops.gemm if wide else ops.gemm_skinny
        if not wide:
            self._dec_in(st, src, x)
        if st.shared is not None:
            self._attn_prefix(cache, st, li)
            ops.attn_decode_fused(st.qkv, cache.k[li], cache.v[li], st.ctx, cache.B, self.H, cache.d_pos, self.rot,
                                  self.sin_t, self.cos_t, pos_stride=cache.pos_stride, shared=st.shared)
        elif st.T > 1:
            ops.attn_decode_chunk(st.qkv, cache.k[li], cache.v[li], st.ctx, cache.B, st.T, self.H, cache.d_pos, self.rot,
                                  self.sin_t, self.cos_t, pos_stride=cache.pos_stride)
        else:
            ops.attn_decode_fused(st.qkv, cache.k[li], cache.v[li], st.ctx, cache.B, self.H, cache.d_pos, self.rot,
                                  self.sin_t, self.cos_t, pos_stride=cache.pos_stride)
        a = G(st.ctx, src.out, out=st.a)
        par = ly.mlp_par is not None or ly.attn_par is not None
        if par and not wide:      # parallel adapters read ln_1(x): the one GEMV-step configuration that needs the LayerNorm as a tensor
            ops.layernorm(x, ly.ln_g, ly.ln_b, self.eps, out=st.ln)
        if ly.attn_adapter is not None:
            a = self._adapter(G, G, ly.attn_adapter, ly.attn_act, ly.attn_ad_ln, st.ln if ly.attn_par is not None else a, ly.attn_par,
                              (a,), t=st.ta[:, : ly.attn_adapter[0].N], ln_out=st.ad_ln, out=st.a2)
        if ly.mlp_adapter is not None:
            G(st.h, src.fc_out, out=st.m)
            self._adapter(G, G, ly.mlp_adapter, ly.mlp_act, ly.mlp_ad_ln, st.ln if ly.mlp_par is not None else st.m, ly.mlp_par,
                          (st.m, a, x), t=st.t[:, : ly.mlp_adapter[0].N], ln_out=st.ad_ln, out=xn)
        else:
            G(st.h, src.fc_out, out=xn, residuals=(a, x))

    def _block_wide(self, cache, st, li, ly, src, x, xn):
        # B > 16 (the weight-streaming GEMV kernels take M <= 16): the generic block, every projection through the tile GEMM
        # on the prefill operands -- weights are still read once per step for the whole batch (reference sampling.py:43-121
        # has no batch limit).  LayerNorm is a launch of its own there (the fold lives in the GEMV kernel)
        ops.layernorm(x, ly.ln_g, ly.ln_b, self.eps, out=st.ln)
        ops.gemm(st.ln, ly.qkv, out=st.qkv)
        ops.gemm(st.ln, ly.fc_in, out=st.h, act=ops.MG_ACT_GELU_NEW)
        self._block_generic(cache, st, li, ly, ly, x, xn, wide=True)

    def _plan_decode(self, B: int):
        """(kind of every layer's block, what decode() refuses this plan with | None) for a cache of B rows under the engine's
        current switches; builds the operands the kinds read, so that no token step allocates."""
        mode = self._quantised_decode()
        w8 = mode is not None           # either quantised format: the blocks take the kinds W8A16 takes
        name, _, kmod, field, _ = mode or ("", "", 0, "", "")
        kinds = [self._block_kind(ly, B > 16, w8, self.fold_dn, self.group_launches) for ly in self.layers]
        if w8 and B > 16:
            return kinds, f"{name} decode covers batches of at most 16 sequences"
        if w8 and self._quant_misfit(mode) is not None:
            return kinds, self._quant_misfit(mode)
        for ly, kind in zip(self.layers, kinds):
            if kind in ("fold1", "fold2"):
                self._ensure_out_up(ly)
            if kind == "v2":
                self._adapter_up_cat(ly)
            # an adapter projection whose K is not a multiple of 1024 (W4A16: 512) has no quantised operand (_ensure_decode_packs_q)
            q = getattr(ly, field) if w8 else None
            if w8 and kind == "grouped" and any(p is None for p in q.mlp_adapter):
                return kinds, (f"{name} decode needs adapter projections with K % {kmod} == 0" +
                               (" (downsample_factor 4 at d = 4096)" if kmod == 1024 else ""))
            if w8 and kind == "v2" and (q.up_cat is None or q.mlp_adapter[0] is None):
                return kinds, f"{name} decode of the MAGMA_v2 step needs adapter projections with K % {kmod} == 0"
        return kinds, None

    def _ensure_decode_state(self, cache: KVCache):
        """The cache's decode state: scratch buffers, captured graphs and the plan of the token step (st.w8 / st.w4, st.kinds, st.refusal),
        fixed when the state is created -- the eager step and every graph captured on this cache run the same launches, whatever
        is written to the engine's switches afterwards.  The captured graphs hold the addresses of one set of adapter operands
        (st.packs_gen): once repack_adapters has replaced them (or the cache has come to another engine) the graphs are dropped
        here, wherever the cache lives -- pool or caller -- and the next steps capture again on the current operands.  The
        scratch buffers, the plan and the selection state stay."""
        self._current_packs()
        st = cache.decode_state
        if st is not None and st.packs_gen != self._packs_gen:
            st.graphs.clear()
            st.packs_gen = self._packs_gen
        if st is None:
            if cache.B <= 16:           # larger batches run the tile GEMM on the prefill operands (no LayerNorm-folded packs)
                self._ensure_decode_packs()
            mode = self._quantised_decode()
            if mode is not None:
                self._ensure_decode_packs_q(mode)
            st = self._alloc_decode_state(cache)
            st.w8, st.w4 = self.decode_w8, self.decode_w4
            st.kinds, st.refusal = self._plan_decode(cache.B)
            st.packs_gen = self._packs_gen
            cache.decode_state = st
        return st

    def _ensure_spec_state(self, cache: KVCache, T: int):
        """The cache's state of the speculative step with T rows per sequence (cache.spec[T]): _ensure_decode_state's scratch and
        plan for B * T rows -- every GEMV of the step sees an ordinary M = B * T operand, the quantised and packed steps
        included --, graphs of its own, and the loop's bookkeeping buffers (ids, draft counts, token counts, statistics, lookup ids)."""
        self._current_packs()
        st = cache.spec.get(T)
        if st is not None and st.packs_gen != self._packs_gen:
            st.graphs.clear()
            st.packs_gen = self._packs_gen
        if st is None:
            B, R, dev = cache.B, cache.B * T, self.device
            if not 2 <= T <= 8 or R > 16:
                raise ValueError(f"a speculative step runs B * T rows through the weight-streaming GEMVs, which take at most 16: got "
                                 f"B * T = {B} * {T} = {R}")
            if cache.prefix_P:
                raise NotImplementedError("speculative decoding is not combined with a shared session prefix")
            self._ensure_decode_packs()
            mode = self._quantised_decode()
            if mode is not None:
                self._ensure_decode_packs_q(mode)
            st = self._alloc_decode_state(cache, rows=R)
            st.T = T
            # MAGMA_SPEC_COLAUNCH (default 1; read when the state is created, like the step's other switches): 0 runs the chunk
            # attention and the co-launched GEMV as two launches -- the GEMV workgroups then keep their own LDS block and registers,
            # the attention no longer hides under the weight stream (tools/speculative_bench.py times both)
            st.colaunch = os.environ.get("MAGMA_SPEC_COLAUNCH", "1") != "0"
            st.w8, st.w4 = self.decode_w8, self.decode_w4
            st.kinds, st.refusal = self._plan_decode(R)
            st.packs_gen = self._packs_gen
            z = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)  # noqa: E731
            st.n_draft, st.count, st.lookup_len, st.stats, st.lookup = z(B), z(B), z(B), z(B, 3), z(B, 0)
            # the sequences' sampler records of a sampled speculative call (ops.sample_rows_table; greedy until a call writes its
            # own): the table's address is a launch argument of the captured step, its contents are not
            st.sample_rows = torch.zeros(B, ops.SAMPLE_ROW_BYTES, dtype=torch.uint8, device=dev)
            st.limit, st.armed = 0, False
            cache.spec[T] = st
        return st

    def decode_chunk(self, input_ids: torch.Tensor, cache: KVCache) -> torch.Tensor:
        """``input_ids`` (B, T), 2 <= T <= 8, B * T <= 16, as T consecutive positions of every sequence in ONE step against the cache
        (chunk attention): fp32 logits (B * T, V), row b * T + t those of position pos_b + t -- what T single-token steps give.
        Eager, teacher-forced: K / V are appended at [pos_b, pos_b + T), the positions do not advance, nothing is selected.  The
        speculative step (_spec_step) runs the same launches."""
        B, T = input_ids.shape
        if B != cache.B:
            raise ValueError(f"the cache holds {cache.B} rows, input_ids {B}")
        if int(cache.rows_pos().max()) - cache.prefix_P + T > cache.Smax:
            raise ValueError(f"KV cache full (Smax={cache.Smax}); pass a larger cache_hint / max_steps")
        st = self._ensure_spec_state(cache, T)
        if st.refusal is not None:
            raise NotImplementedError(st.refusal)
        st.ids.copy_(input_ids.reshape(B * T, 1))
        self._step_logits(cache, st, st.ids)
        return st.logits[:, : self.V]

    def _decode_speculate(self, cache: KVCache, plan: SelectionPlan, use_graph: bool = True):
        """One speculative step of a loop armed by _arm_speculate; the captured graphs live in cache.spec[T]."""
        T = plan.mode[1]
        st = cache.spec.get(T)
        if st is None or not st.armed or cache.finish is None or not cache.ragged:
            raise ValueError("speculative decoding needs a cache armed for this T (prefill with eos_token= and a speculative plan)")
        self._current_packs()
        if st.packs_gen != self._packs_gen:
            st.graphs.clear()
            st.packs_gen = self._packs_gen
        key = (plan.graph_key(True), st.limit, st.lookup.shape[1])
        if not use_graph:
            self._spec_step(cache, st, plan)
        elif key in st.graphs:
            st.graphs[key].replay()
        elif st.steps == 0:
            self._spec_step(cache, st, plan)              # first step eager (loads code objects)
        else:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._spec_step(cache, st, plan)
            st.graphs[key] = g
            g.replay()
        st.steps += 1
        cache.pos += T          # an upper bound: the rows' own positions are on the device until speculate_results reads them
        return st.logits[:, : self.V], st.token

    def speculate_results(self, cache: KVCache, T: int):
        """After a speculative loop: (count int64 [B] of every row's emitted tokens, stats int64 [B, 3] = steps, drafted, accepted),
        on the host; the one read-back of the loop, which also makes the host mirror of the positions exact again."""
        st = cache.spec[T]
        pos, count, stats = cache.d_pos.cpu(), st.count.cpu(), st.stats.cpu()
        cache.set_rows(pos.to(torch.int64))
        st.armed = False
        return count.to(torch.int64), stats.to(torch.int64)

    def decode(self, input_ids: Optional[torch.Tensor], cache: KVCache, use_graph: bool = True, sampling=None, select: bool = True,
               beam=None, processors=None, stop=None, logprobs=None, constraint=None, guidance=None, plan=None):
        """One cached step.  Returns (fp32 logits (B,V) view, selected token (B,) view: greedy, or sampled when
        ``sampling = (temperature, top_k, top_p)`` or ``("warp", temperature, top_k, top_p, min_p)``, sample_mode); both are
        overwritten by the next step.  ``input_ids=None`` feeds the
        previously selected tokens back without leaving the device.  ``select=False`` (teacher-forced positions of a
        multi-token call): no token is selected -- the history, the RNG step counter and the all-eos latch are left alone,
        only the KV write position advances; the returned token view is stale.
        ``plan`` (forward): the SelectionPlan of the loop, INSTEAD of the selection keywords; a replayed step then checks nothing.
        ``processors`` (forward): the logits processors run in place on the step's logits before the selection, so the
        returned logits are then the PROCESSED ones (beam search: the processed log_softmax scores).
        ``stop`` (forward): per-row stopping -- the cache must have been armed with it (its finish record reset) by the prefill /
        extend call; the returned token view holds the pad id for rows that had finished.
        ``logprobs`` (forward): the step also writes column step of the cache's log-probability buffers, from the RAW logits; with
        ``processors`` too, those and the selection run on a second buffer, whose rows are what is returned.
        ``constraint`` (forward): the trie constraint in the processors' launch; it counts as one of them in all of the above.
        ``guidance`` (forward): the cache's 2R rows are R pairs; the returned token view holds the R selected tokens twice, the
        returned logits hold the guided rows [0, R) in place of the conditional ones."""
        if plan is None:
            plan = self.selection_plan(sampling=sampling, beam=beam, processors=processors, stop=stop, logprobs=logprobs,
                                       constraint=constraint, guidance=guidance, vocab=self.V)
        if plan.is_speculate:
            if input_ids is not None or not select:
                raise ValueError("a speculative step feeds its own ids back: decode(None, cache, plan=plan)")
            return self._decode_speculate(cache, plan, use_graph)
        if cache.pos - cache.prefix_P >= cache.Smax:
            raise ValueError(f"KV cache full (Smax={cache.Smax}); pass a larger cache_hint / max_steps")
        if cache.B > 16:
            use_graph = False       # the tile-GEMM step of large batches is launched eagerly (split-K scratch is per stream)
            if not getattr(self, "_warned_wide", False):
                self._warned_wide = True
                import warnings
                warnings.warn(f"decode batch {cache.B} > 16: the token step runs every projection through the tile GEMM, launched "
                              "eagerly with a separate LayerNorm (correct, tested) -- the weight-streaming GEMVs, the fused "
                              "launches and the captured hipGraph of the B <= 16 step do not apply, and W8A16 / W4A16 decode is refused",
                              RuntimeWarning, stacklevel=2)
        st = self._ensure_decode_state(cache)
        if st.refusal is not None:      # before anything of the step is enqueued
            raise NotImplementedError(st.refusal)
        feed_back = input_ids is None
        if not feed_back:
            st.ids.copy_(input_ids.reshape(cache.B, 1))
        if not select:
            if feed_back:
                raise ValueError("decode(select=False) needs input_ids: there is no selected token to feed back")
            plan = plan.without_selection()
        plan.arm(cache, st)
        key = plan.graph_key(feed_back)
        if not use_graph:
            self._decode_step(cache, st, plan, feed_back)
        elif key in st.graphs:
            st.graphs[key].replay()
        elif st.steps == 0:
            self._decode_step(cache, st, plan, feed_back)    # first step eager (loads code objects)
        else:
            g = torch.cuda.CUDAGraph()            # hipGraph on ROCm
            with torch.cuda.graph(g):
                self._decode_step(cache, st, plan, feed_back)
            st.graphs[key] = g
            g.replay()
        st.steps += 1
        cache.pos += 1
        return (st.logits_proc if plan.second_buffer else st.logits)[:, : self.V], st.token

    # ------------------------------------------------- loss (eval) forward
    def forward_loss(self, embeds: torch.Tensor, labels: torch.Tensor, want_hidden=False, want_logits=False) -> LMOutput:
        """Shifted cross-entropy of the full sequence (reference magma.py:270-274).
        lm_head + CE are evaluated only on rows that carry a target (the others
        contribute nothing to the loss); inference-mode forward, see train engine
        for the autograd version."""
        B, S, _ = embeds.shape
        x, hs = self._blocks_prefill(embeds, None, want_hidden)
        labels = labels.to(self.device)
        head = self._target_logits(x, S, labels[:, 1:])
        if head is None:
            return LMOutput(loss=torch.full((), float("nan"), device=self.device), logits=None, hidden_states=hs,
                            past_key_values=None)
        target_rows, kept, target_logits = head
        loss, _ = ops.cross_entropy(target_logits, kept)
        # reference magma.py:270-276 .logits: (B, S, V) over every position -- on request now, otherwise on first access
        full = (self._full_logits(x, B * S).view(B, S, self.V) if want_logits
                else LMOutput.lazy(lambda: self._full_logits(x, B * S).view(B, S, self.V)))
        return LMOutput(loss=loss, logits=full, hidden_states=hs, past_key_values=None,
                        target_rows=target_rows, target_logits=target_logits)

    def _target_logits(self, x: torch.Tensor, S: int, tgt: torch.Tensor):
        """ln_f and the fp32 head on the rows that predict a target, the ONE row selection of forward_loss and score.  ``x``
        (B * S, d) the blocks' output; ``tgt`` (B, n <= S) int64 on the device: the token position s of row b predicts, -100 for
        none.  Returns (rows of x [n_kept] in (b, s) order, their targets [n_kept], logits (n_kept, V) fp32 view), or None when no
        position carries a target.  Targets outside [0, V) raise (ops.refuse_targets_outside)."""
        B, n = tgt.shape
        flat = tgt.reshape(-1)
        rows = (torch.arange(B, device=self.device)[:, None] * S + torch.arange(n, device=self.device)[None, :]).reshape(-1)
        keep = (flat != -100).nonzero().squeeze(1)           # host sync: index plumbing only
        if keep.numel() == 0:
            return None
        kept = flat[keep].contiguous()
        ops.refuse_targets_outside(kept, self.V)            # one more two-element device-to-host copy, next to the sync ``keep`` paid
        xr = x.index_select(0, rows[keep])
        xl = ops.layernorm(xr, self.lnf_g, self.lnf_b, self.eps)
        logits = torch.empty(xl.shape[0], self.Vp, dtype=torch.float32, device=self.device)
        ops.gemm(xl, self.head, out=logits)
        return rows[keep], kept, logits[:, : self.V]

    @staticmethod
    def check_key_scale(key_scale, B: int, S: int) -> torch.Tensor:
        """The host check of a key scale, before any launch: a (B, S) tensor, finite, >= 0.  Returns it as a contiguous fp32 host
        tensor (the caller moves it to the device)."""
        ks = torch.as_tensor(key_scale)
        if ks.ndim != 2 or tuple(ks.shape) != (B, S):
            raise ValueError(f"key_scale must have shape ({B}, {S}), got {tuple(ks.shape)}")
        if not ks.dtype.is_floating_point:
            raise ValueError(f"key_scale must be a floating-point tensor, got {ks.dtype}")
        ks = ks.detach().to("cpu", torch.float32).contiguous()       # one small copy when it sat on the device
        if not bool(torch.isfinite(ks).all()):
            raise ValueError("key_scale must be finite")
        if bool((ks < 0).any()):
            raise ValueError("key_scale must be >= 0")
        return ks

    def score(self, embeds: torch.Tensor, tgt: torch.Tensor, n_top: int = 0, key_scale=None):
        """Log-probabilities of given tokens (Magma.score; DESIGN.md "Token log-probabilities"): one cache-less forward over
        ``embeds`` (B, S, d), the fp32 head on the rows that predict a target (``tgt`` (B, S) int64: the token position s of row
        b predicts, -100 for none; _target_logits), then the kernel of the generate() loop without a step counter.  Returns device
        tensors in (b, s) order of the targets: (log-probabilities [n], top ids [n, n_top] int32, their log-probabilities
        [n, n_top]).  ``key_scale`` (B, S), finite and >= 0 (checked on the host before any launch): the attention of every block and
        head multiplies the score of key j of row b by key_scale[b, j] (DESIGN.md "Explaining an answer"); None launches what it
        always did."""
        n_top = self.logprob_mode(n_top, self.V)
        B, S, _ = embeds.shape
        if key_scale is not None:
            if self.fp8_mode and self.fp8_attn:
                raise NotImplementedError("key_scale is not implemented for the fp8 attention mode")
            key_scale = self.check_key_scale(key_scale, B, S).to(self.device)
        x, _ = self._blocks_prefill(embeds, None, key_scale=key_scale)
        head = self._target_logits(x, S, tgt.to(self.device))
        if head is None:
            raise ValueError("score: no position carries a target")
        _, kept, logits = head
        n = kept.numel()
        lp = torch.empty(n, 1, dtype=torch.float32, device=self.device)
        top_id = torch.empty(n, 1, n_top, dtype=torch.int32, device=self.device)
        top_lp = torch.empty(n, 1, n_top, dtype=torch.float32, device=self.device)
        ops.token_logprobs(logits, kept, lp, top_id if n_top else None, top_lp if n_top else None)
        return lp[:, 0], top_id[:, 0], top_lp[:, 0]


class SlotSession:
    """Generation over a stream of requests (DESIGN.md "Request streams"; sampling.generate_stream): ``slots`` rows generate in
    one captured token step, and the row of a request that has finished is handed to the next request while the others keep
    generating.  The session owns a private ragged KVCache (never pooled, never handed out) and a staging cache of
    ``admit_rows`` rows; it runs rounds of
      harvest  one host look (one blocking copy) at the finish record and the ring history: every newly finished row gives its
               tokens;
      admit    up to as many requests as slots are free are pulled, prefilled in passes of the FIXED shape (admit_rows, S_stage)
               -- so a request's bits do not depend on what was admitted with it --, their first tokens selected from the staged
               logits and installed with one ops.slots_admit launch per pass;
      step     ``every`` replays of the captured token step under ``plan`` (plan.slots).
    The host mirrors every slot's occupant, begin column and position bound by counting the steps it enqueued: nothing but the
    harvest reads the device.
    Sampled selection: a token step draws from the Philox counter (state[0] = 1 + steps enqueued, slot), as every generate() loop
    does; the first token of a request is drawn at its admission from a counter domain of its own, (admit_counter(pass), staging
    row) with admit_counter(p) = -1 - p -- as the kernel's unsigned counter word 2^32 - 1 - p, which no token step reaches -- so
    no two draws of a session share a counter (draw_counters is the host statement of which ones a schedule uses).
    Per-request sampling (plan.is_rows; DESIGN.md "Per-request sampling"): an item carries its own record (temperature, top_k, top_p,
    min_p, seed) as its fourth entry.  The admission draws the first tokens with ops.sample_rows over the staging rows at counter 0
    under a staging table (unused staging rows are greedy) and copies every admitted request's record into its slot's row of the
    live table -- outside the captured step, before the next replay --; a token step draws row b at its occupant's own token index
    under that record.  A request's draws then depend on its seed and its logits alone: admit_counter and draw_counters describe
    the session-wide mode only.
    Session prefix (``prefix``: (P, d) embeddings or a one-row KVCache that is only read): its K / V positions [0, P) are put into
    every live slot and every staging row ONCE, at set-up (plain copies, as KVCache.expand); an admission pass then runs the
    cached-append prefill of LMEngine.extend over the same fixed (admit_rows, S_stage) rows behind them -- every staging row's
    write position is reset to P on the device first -- and ops.slots_admit(pos0=P) moves positions [P, P + len) only, so a slot
    keeps its prefix over any number of occupants.  Nothing is ever re-allocated: the captured step stays valid.
    ``share_prefix`` (DESIGN.md "Shared session prefix"): the live cache holds the rows' OWN positions only, slots x
    ceil64(max_prompt + max_new) -- it carries ONE copy of the prefix (KVCache.prefix_k / prefix_v) that every block's prefix
    launch reads for all rows --, ops.slots_admit(pos0=P, dst0=0) moves staged positions [P, P + len) to own indices [0, len), and
    every d_pos starts at P.  The staging rows keep their own copies: admission is as above.
    Rules, constraint, log-probabilities (DESIGN.md "Choosing over a request stream"; sampling.choose_stream): under a plan built
    with ``processors`` / ``constraint=True`` / ``logprobs`` the token step's launches are the slot entry points, which read every
    row's OWN tokens -- its window of the ring -- and skip idle rows.  An item then carries its TokenTrie; the admission selects the
    first token after the step-0 rules and the root mask (the flat kernels over the staging rows), writes column 0 of the slot's
    log-probability row from the raw staged logits and installs the slot's root; the device table is the forest of the live slots'
    tries (_install_tries); the harvest returns a finished row's log-probability columns with its tokens, in the same one copy."""

    @staticmethod
    def admit_counter(n_pass: int) -> int:
        """The value of state[0] the first tokens of admission pass ``n_pass`` (0, 1, ...) are drawn under."""
        return -1 - int(n_pass)

    @staticmethod
    def draw_counters(schedule):
        """[(unsigned 32-bit counter word, row)] of every draw of a session, in order: ``schedule`` lists ("admit", staging rows
        used) and ("step", slots) events as the session enqueues them.  Host statement of the counters, for checking that they
        are unique."""
        out, steps, passes = [], 0, 0
        for kind, rows in schedule:
            if kind == "admit":
                out += [(SlotSession.admit_counter(passes) & 0xffffffff, j) for j in range(rows)]
                passes += 1
            else:
                out += [((1 + steps) & 0xffffffff, b) for b in range(rows)]
                steps += 1
        return out

    def __init__(self, engine: "LMEngine", plan: SelectionPlan, *, slots: int, max_new: int, max_prompt: int, every: int,
                 admit_rows: int, seed: Optional[int] = None, prefix=None, share_prefix: bool = False,
                 trie_capacity: Optional[int] = None):
        if not plan.slots or plan.stop is None:
            raise ValueError("a slot session runs under a plan built with slots=True and per-row stopping")
        if not 1 <= slots <= ops.SLOTS_MAX or not 1 <= admit_rows <= slots or max_new < 1 or max_prompt < 1 or every < 1:
            raise ValueError(f"need 1 <= admit_rows <= slots <= {ops.SLOTS_MAX} and max_new, max_prompt, every >= 1")
        n_pos = engine.cfg.max_position_embeddings
        self.S_stage = ops.ceil_to(max_prompt, 64)
        self.P = P = self.prefix_rows(engine, prefix)
        if share_prefix and not P:
            raise ValueError("share_prefix=True needs a prefix: there is nothing to share")
        self.shared = bool(share_prefix)
        if P + max_prompt + max_new > n_pos or P + self.S_stage > n_pos:
            raise ValueError((f"a prefix of {P} rows + " if P else "") + f"max_prompt = {max_prompt} (staged as {self.S_stage} rows) + "
                             f"max_new_tokens = {max_new} exceeds max_position_embeddings = {n_pos}")
        dev = engine.device
        self.engine, self.plan, self.B, self.every, self.n_admit = engine, plan, slots, every, admit_rows
        self.max_new, self.max_prompt = max_new, max_prompt
        self.cache = cache = KVCache(engine.L, slots, engine.H, ops.ceil_to((0 if self.shared else P) + max_prompt + max_new, 64), dev,
                                     ragged=True)
        if self.shared:         # before the decode state: it sizes the partials scratch from the cache
            cache.prefix_P = P
            cache.prefix_k = torch.empty(engine.L, 1, engine.H, P, 256, dtype=BF16, device=dev)
            cache.prefix_v = torch.empty(engine.L, 1, engine.H, P, 256, dtype=BF16, device=dev)
        self.stage = KVCache(engine.L, admit_rows, engine.H, P + self.S_stage, dev, ragged=True)
        self.stage_in = torch.zeros(admit_rows, self.S_stage, engine.d, dtype=BF16, device=dev)
        self.first = torch.zeros(admit_rows, dtype=torch.int64, device=dev)
        self.admit_state = torch.tensor([-1, -1], dtype=torch.int32, device=dev)      # {admit_counter(pass), unused}: the admissions' draws
        self.passes = 0                 # admission passes enqueued
        # the ring holds a finished row's tokens until the next harvest, at most ``every`` steps later: Hc >= max_new + every
        self.Hc = 1 << (max_new + every - 1).bit_length()
        assert self.Hc >= max_new + every
        cache.ring_cols, cache.eos = self.Hc, int(plan.stop[0][0])
        cache.sample_state.copy_(torch.tensor([1, -1], dtype=torch.int32), non_blocking=True)    # column (state[0] - 1) exists
        if seed is not None and not plan.is_rows:
            cache.seed.fill_(int(seed) & 0x7fffffffffffffff)
        if plan.is_rows:
            if plan.cons is not None:
                raise NotImplementedError("per-request sampler settings are not combined with a constrained slot plan")
            self.stage_rows = torch.zeros(admit_rows, ops.SAMPLE_ROW_BYTES, dtype=torch.uint8, device=dev)
        self.st = engine._ensure_decode_state(cache)
        if self.st.refusal is not None:
            raise NotImplementedError(self.st.refusal)
        # choosing over a stream (DESIGN.md "Choosing over a request stream"): the rules, the constraint and the log-probabilities
        # of a slot plan.  The admission runs the FLAT kernels over the staging rows at step 0 (zero_state) -- their roots, path and
        # column-0 buffers are the stage_* ones --; the live side's table is the forest of the live slots' tries (_install_tries)
        i32 = torch.int32
        self.zero_state = torch.tensor([0, -1], dtype=i32, device=dev)
        self.stage_hist = torch.zeros(admit_rows, 1, dtype=torch.int64, device=dev)       # (step 0 reads no column of it)
        self.slot_trie = [None] * slots         # per slot: its occupant's TokenTrie
        self.root_of, self.roots_held = {}, None  # id(trie) -> its root in the device table; the roots the device holds
        if plan.cons is not None:
            cache.alloc_trie((int(trie_capacity) + 1) // 2 if trie_capacity else 1)      # (alloc_trie doubles what it is asked for)
            self.stage_roots = torch.zeros(admit_rows, dtype=i32, device=dev)
            self.stage_path = ops.trie_path(admit_rows, dev)
        if plan.n_top is not None:
            cache.lp_cols = max_new
            self.stage_lp = torch.zeros(admit_rows, 1, dtype=torch.float32, device=dev)
            self.stage_top_id = torch.zeros(admit_rows, 1, plan.n_top, dtype=i32, device=dev)
            self.stage_top_lp = torch.zeros(admit_rows, 1, plan.n_top, dtype=torch.float32, device=dev)
        plan.arm(cache, self.st, first=True)
        # every slot starts finished and idle at position 0 (shared prefix: at P, own index 0)
        cache.finish.copy_(torch.tensor([[0, ops.STOP_LEN]] * slots, dtype=torch.int32), non_blocking=True)
        cache.d_pos.fill_(P if self.shared else 0)
        self.steps = 0                  # token steps enqueued: the device's state[0] is 1 + steps
        self.occ = [None] * slots       # per slot: (request index, begin column, prompt length, limit, steps at admission)
        if P:
            self._install_prefix(prefix)

    @staticmethod
    def prefix_rows(engine: "LMEngine", prefix) -> int:
        """The number of rows P of a session prefix (0: none), after checking that the session can take it: (P, d) embeddings of
        the engine's width, or this engine's one-row KVCache with nothing pending that no beam or contrastive search ran on."""
        if prefix is None:
            return 0
        if isinstance(prefix, KVCache):
            if prefix.B != 1:
                raise ValueError(f"the prefix cache holds {prefix.B} rows: a session has ONE prefix (cache it alone)")
            if prefix.pending is not None and bool((prefix.pending >= 0).any()):
                raise ValueError("the prefix cache holds a token that has not been fed back: a prefix ends at a cached position")
            if (prefix.beam is not None and prefix.beam.k > 1) or prefix.contrast is not None:
                raise ValueError("a beam-search or contrastive-search cache cannot be a session prefix")
            owner = prefix.owner() if prefix.owner is not None else None
            if (owner is not None and owner is not engine) or (len(prefix), prefix.k.shape[2]) != (engine.L, engine.H) \
                    or prefix.k.device != engine.wte.device:
                raise ValueError("the prefix cache belongs to another engine")
            P = int(prefix.rows_pos()[0])
        elif torch.is_tensor(prefix):
            if prefix.ndim != 2 or prefix.shape[1] != engine.d:
                raise ValueError(f"the prefix must be (P, {engine.d}) embeddings, got {tuple(prefix.shape)}")
            P = prefix.shape[0]
        else:
            raise ValueError(f"the prefix is embeddings or a KVCache, got {type(prefix).__name__}")
        if P < 1:
            raise ValueError("the prefix is empty")
        return P

    @torch.no_grad()
    def _install_prefix(self, prefix):
        """Set-up, once: the prefix's K / V positions [0, P) of every layer and head into every live slot and every staging
        row.  A given cache is only read; embeddings are prefilled once, alone, as Magma.cache_prompt does."""
        P = self.P
        if not isinstance(prefix, KVCache):
            lens = torch.tensor([P], dtype=torch.int64)
            _, prefix, _ = self.engine.prefill(prefix[None].to(self.engine.device), 0, lengths=lens)
        if self.shared:         # the live side keeps the one copy
            self.cache.prefix_k.copy_(prefix.k[:, :, :, :P])
            self.cache.prefix_v.copy_(prefix.v[:, :, :, :P])
        for own in (self.stage,) if self.shared else (self.cache, self.stage):
            own.k[:, :, :, :P].copy_(prefix.k[:, :, :, :P])
            own.v[:, :, :, :P].copy_(prefix.v[:, :, :, :P])

    def _bound(self, o) -> int:
        """The largest position the occupant's row can be at now."""
        return self.P + o[2] + min(self.steps - o[4], o[3] - 1)

    @torch.no_grad()
    def _install_tries(self, batch, slots):
        """The tries of an admission pass: the device table is the forest of the live slots' tries (sampling.trie_forest: one
        entry per OBJECT), rebuilt and copied only when the pass brings a trie the table does not hold; a table that outgrows the
        buffer re-allocates it, which drops the captured constrained steps (KVCache.alloc_trie).  A rebuild renumbers the nodes:
        every live slot's root is rewritten, and what its path cache holds fails its proof and is walked again.  The roots are
        copied only when they differ from what the device holds.  Returns the staging rows' roots.  Enqueue-only."""
        from .sampling import trie_forest
        cache = self.cache
        for it, b in zip(batch, slots):
            self.slot_trie[b] = it[3]
        if any(id(it[3]) not in self.root_of for it in batch):
            live = [t for t in self.slot_trie if t is not None]
            table, roots = trie_forest(live)
            cache.alloc_trie(table.numel())
            cache.trie_table[: table.numel()].copy_(table, non_blocking=True)
            self.root_of = {id(t): int(r) for t, r in zip(live, roots.tolist())}
            self.tries_held = live              # (the objects stay alive: their ids key root_of)
        roots = [0 if t is None else self.root_of[id(t)] for t in self.slot_trie]
        if roots != self.roots_held:
            cache.trie_roots.copy_(torch.tensor(roots, dtype=torch.int32), non_blocking=True)
            self.roots_held = roots
        return [self.root_of[id(it[3])] for it in batch] + [0] * (self.n_admit - len(batch))

    def _select_first(self, logits, batch, slots):
        """The first tokens of an admission pass into self.first, from the staged logits (n_admit, V): the plan's rules at step 0
        and the root mask of every staging row's own trie, by the flat kernels on a copy; then -- from the RAW logits -- column 0
        of the slots' log-probability rows.  Enqueue-only."""
        plan, cache, n = self.plan, self.cache, len(batch)
        mode, proc, stop, n_top, cons = plan[:5]
        raw = logits
        if plan.rewrites_logits:
            logits = logits.clone() if n_top is not None else logits
            more = {} if len(stop[0]) < 2 else dict(eos_more=cache.stop_table[1:ops.STOP_MAX_EOS], n_eos_more=len(stop[0]) - 1)
            rules = proc if proc is not None else (1.0, 0, 0, ())
            kw = dict(repetition_penalty=rules[0], no_repeat_ngram_size=rules[1], min_new_tokens=rules[2], eos=cache.eos,
                      suppress=cache.suppress, n_suppress=len(rules[3]), **more)
            if cons is not None:
                self.stage_roots.copy_(torch.tensor(self._install_tries(batch, slots), dtype=torch.int32), non_blocking=True)
                ops.logits_process_constrained(logits, self.zero_state, self.stage_hist, cache.trie_table, self.stage_roots,
                                               self.stage_path, **kw)
            else:
                ops.logits_process(logits, self.zero_state, self.stage_hist, **kw)
        if mode is None:
            ops.argmax(logits, out=self.first)
        elif plan.is_rows:      # every request under its own record at counter 0 -- its solo call's first draw; then the records go live
            recs = [it[3] for it in batch] + [(0.0, 0, 0.0, 0.0, 0)] * (self.n_admit - n)
            self.stage_rows.copy_(ops.sample_rows_table(*zip(*recs)), non_blocking=True)
            ops.sample_rows(logits, self.stage_rows, self.zero_state, mode[1], out=self.first)
            at = torch.tensor(slots, dtype=torch.int64).to(logits.device, non_blocking=True)
            cache.sample_rows.index_copy_(0, at, self.stage_rows[:n])
        else:       # a counter domain of its own: the token steps draw under state[0] = 1, 2, ..., never under a negative value
            self.admit_state[:1].fill_(self.admit_counter(self.passes))
            if mode[0] == "warp":
                ops.sample_warp(logits, mode[1], mode[2], mode[3], mode[4], cache.seed, self.admit_state, out=self.first)
            else:
                ops.sample(logits, mode[0], mode[1], mode[2], cache.seed, self.admit_state, out=self.first)
        if n_top is not None:
            ops.token_logprobs(raw, self.first, self.stage_lp, self.stage_top_id if n_top else None,
                               self.stage_top_lp if n_top else None)
            at = torch.tensor(slots, dtype=torch.int64).to(raw.device, non_blocking=True)
            cache.lp[:, 0].index_copy_(0, at, self.stage_lp[:n, 0])
            if n_top:
                cache.top_id[:, 0].index_copy_(0, at, self.stage_top_id[:n, 0])
                cache.top_lp[:, 0].index_copy_(0, at, self.stage_top_lp[:n, 0])

    @torch.no_grad()
    def _admit(self, batch, slots):
        """One staging pass: ``batch`` = [(index, (S, d) embeddings, limit[, TokenTrie])] goes to the free ``slots`` (as many)."""
        eng, cache, n = self.engine, self.cache, len(batch)
        self.stage_in.zero_()
        lens = [1] * self.n_admit       # unused staging rows: one zero row
        for j, (_, emb, *_) in enumerate(batch):
            lens[j] = emb.shape[0]
            self.stage_in[j, : lens[j]].copy_(emb)
        if self.P:      # behind the prefix: LMEngine.extend's cached-append prefill, every staging row's write position back at P
            self.stage.d_pos.fill_(self.P)
            x, _ = eng._blocks_prefill(self.stage_in, self.stage, chunk=True)
        else:
            x, _ = eng._blocks_prefill(self.stage_in, self.stage)
        rows = (torch.arange(self.n_admit, dtype=torch.int64) * self.S_stage + torch.tensor(lens) - 1).to(eng.device, non_blocking=True)
        logits = eng._head(ops.layernorm(x.index_select(0, rows), eng.lnf_g, eng.lnf_b, eng.eps))
        self._select_first(logits, batch, slots)
        self.passes += 1
        stop = self.plan.stop
        ops.slots_admit(self.stage.k, self.stage.v, cache.k, cache.v, list(range(n)), slots, lens[:n], self.first,
                        [it[2] for it in batch], cache.sample_state, cache.d_pos, self.st.token, cache.finish, cache.slot_table,
                        cache.ring, cache.stop_table, len(stop[0]), len(stop[1]), pos0=self.P, dst0=0 if self.shared else None)
        for j, (index, _, limit, *_) in enumerate(batch):
            self.occ[slots[j]] = (index, self.steps % self.Hc, lens[j], limit, self.steps)

    @torch.no_grad()
    def _step(self):
        self.cache.pos = max([self._bound(o) for o in self.occ if o is not None] + [0])
        self.engine.decode(None, self.cache, plan=self.plan)
        self.steps += 1

    def _harvest(self):
        """[(request index, int64 CPU tokens, finish code, slot)] of the rows that have finished since the last look -- under a plan
        with log-probabilities, followed by (lp [count], top ids [count, n_top], top lp [count, n_top]) of the row's columns."""
        if all(o is None for o in self.occ):
            return []
        # the one sync of a round: the finish record, the ring and -- as their bits -- the log-probability rows in one blocking copy
        cache, n_top = self.cache, self.plan.n_top
        parts = [cache.finish.view(-1).to(torch.int64), cache.ring.view(-1)]
        if n_top is not None:
            parts += [t.view(torch.int32).view(-1).to(torch.int64) for t in (cache.lp, cache.top_id, cache.top_lp)]
        both = torch.cat(parts).cpu()
        fin, ring = both[: 2 * self.B].view(self.B, 2), both[2 * self.B: 2 * self.B + self.B * self.Hc].view(self.B, self.Hc)
        if n_top is not None:
            rest, n = both[2 * self.B + self.B * self.Hc:].to(torch.int32), self.B * self.max_new
            lp = rest[:n].view(torch.float32).view(self.B, self.max_new)
            top_id = rest[n: n + n * n_top].view(self.B, self.max_new, n_top)
            top_lp = rest[n + n * n_top:].view(torch.float32).view(self.B, self.max_new, n_top)
        done = [b for b, o in enumerate(self.occ) if o is not None and int(fin[b, 0]) >= 0]
        out = []
        for b in done:
            index, begin = self.occ[b][:2]
            count = (int(fin[b, 0]) % self.Hc - begin) % self.Hc + 1
            cols = (begin + torch.arange(count)) % self.Hc
            item = (index, ring[b, cols].clone(), int(fin[b, 1]), b)
            if n_top is not None:
                item += ((lp[b, :count].clone(), top_id[b, :count].to(torch.int64), top_lp[b, :count].clone()),)
            out.append(item)
            self.occ[b], self.slot_trie[b] = None, None
        return out

    def run(self, requests):
        """Yield (request index, tokens, finish code, slot[, log-probabilities: _harvest]) in completion order.  ``requests`` yields
        (index, (S, d) embeddings on the engine's device, limit[, TokenTrie: under a constrained plan; or the request's sampler record
        (temperature, top_k, top_p, min_p, seed): under a per-row plan]), is pulled lazily -- one item when a slot frees.  When it raises, nothing more is pulled, the
        requests pulled before it are admitted and every row in flight is generated to its end and yielded; then the error is
        raised: no request in front of the failing one is lost."""
        it, exhausted, error = iter(requests), False, None
        while True:
            yield from self._harvest()
            free = [b for b in range(self.B) if self.occ[b] is None]
            while free and not exhausted:
                batch = []
                while len(batch) < min(len(free), self.n_admit):
                    try:
                        batch.append(next(it))
                    except StopIteration:
                        exhausted = True
                        break
                    except Exception as e:  # noqa: BLE001  (raised again once the rows in flight are done)
                        exhausted, error = True, e
                        break
                if batch:
                    self._admit(batch, free[: len(batch)])
                    free = free[len(batch):]
            if all(o is None for o in self.occ):
                if error is not None:
                    raise error
                return
            for _ in range(self.every):
                self._step()
