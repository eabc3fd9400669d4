"""Tensor-level wrappers over the C ABI.  PyTorch is used for device memory,
streams and one-off weight re-layout only; every hot-path computation below is
a call into libmagma_hip.so.  No CPU path exists: tensors must be on a GPU."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

from . import lib as L
from .lib import (MG_A_CONV3X3, MG_A_DENSE, MG_ACT_GELU_NEW, MG_ACT_NONE, MG_ACT_QUICK_GELU, MG_ACT_RELU, MG_AUX_GELU_GRAD,
                  MG_AUX_MUL, MG_AUX_NONE, MG_AUX_QUICK_GELU_GRAD, MG_AUX_RELU_GATE, MG_W_FRAGTILED, MG_W_ROWMAJOR, Epilogue, GemmDesc,
                  SkinnyDesc, check)

BF16 = torch.bfloat16
_zero_pages = {}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*ts):
    """Every op launches on the CURRENT device and its current stream (_stream): operands on a CPU, or on a GPU
    that is not the current one, are refused instead of faulting / silently peer-accessing (Magma.__init__ and the
    entry points of Magma / MagmaEngine make the model's device current)."""
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise L.MagmaHipError(
                "magma_amd ops run on MI355X only (tensor on %s); there is no CPU fallback" % t.device)
        if t.device.index != torch.cuda.current_device():
            raise L.MagmaHipError("tensor on %s but the current HIP device is cuda:%d: wrap the call in "
                                  "torch.cuda.device(tensor.device)" % (t.device, torch.cuda.current_device()))


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def zero_page(device) -> torch.Tensor:
    key = str(device)
    if key not in _zero_pages:
        _zero_pages[key] = torch.zeros(256, dtype=BF16, device=device)
    return _zero_pages[key]


def ceil_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class PackedLinear:
    """A [N, K] weight in the layouts the GEMM kernels consume.

    ``ft``: fragment-tiled [ceil(N/16)][Kp/32][64 lanes][8] (MG_W_FRAGTILED): one
            wave instruction reads 1 KiB contiguous == one MFMA operand fragment.
            Used by the decode (weight-streaming) kernel and by the tile GEMM.
    ``rm``: row-major [N, Kp], K zero-padded to a multiple of 64 (trainable
            weights that change every step keep this cheap layout).
    """

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                 tiled: bool = True, rowmajor: bool = False):
        _need_gpu(weight)
        assert weight.ndim == 2
        self.N, self.K = weight.shape
        if self.K % 8:
            raise ValueError("K must be a multiple of 8")
        self.Kp = ceil_to(self.K, 64)
        self.device = weight.device
        self.ft = None
        self.rm = None
        self.bias = None if bias is None else bias.detach().to(torch.float32).contiguous()
        w = weight.detach().to(BF16)
        if rowmajor:
            self.rm = self._pad(w, self.N, self.Kp)
        if tiled:
            self.ft = self.tile(self._pad(w, ceil_to(self.N, 16), self.Kp))

    @staticmethod
    def _pad(w, n, k):
        if w.shape == (n, k):
            return w.contiguous()
        out = torch.zeros(n, k, dtype=BF16, device=w.device)
        out[: w.shape[0], : w.shape[1]] = w
        return out

    def rows(self, n0: int, n1: int, bias: Optional[torch.Tensor] = None) -> "PackedLinear":
        """Output channels [n0, n1) of this weight as a PackedLinear that SHARES its storage (n0 % 16 == 0: whole row tiles of
        the fragment-tiled layout are contiguous)."""
        assert n0 % 16 == 0 and 0 <= n0 < n1 <= self.N and (n1 % 16 == 0 or n1 == self.N)
        v = PackedLinear.__new__(PackedLinear)
        v.N, v.K, v.Kp, v.device = n1 - n0, self.K, self.Kp, self.device
        v.ft = None if self.ft is None else self.ft[n0 // 16: (n1 + 15) // 16]
        v.rm = None if self.rm is None else self.rm[n0:n1]
        v.bias = bias
        return v

    @staticmethod
    def tile(w: torch.Tensor) -> torch.Tensor:
        n, k = w.shape
        return w.view(n // 16, 16, k // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()

    @staticmethod
    def untile(ft: torch.Tensor) -> torch.Tensor:
        nt, ks = ft.shape[0], ft.shape[1]
        return ft.view(nt, ks, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(nt * 16, ks * 32)


def _epilogue(out: Optional[torch.Tensor], N: int, bias, scale, act, residuals, act_after, aux=None, aux_mode=MG_AUX_NONE,
              aux_after=False, out2=None, mx_out=None, M: int = 0) -> Epilogue:
    """``mx_out`` = (q [M, ceil(N / 128) * 128] uint8, scales uint8 [mg_mx_scale_bytes(M, N)]) from ``mx_empty``: the epilogue also
    writes the OCP MX e4m3 copy of its final value (mg_epilogue.C8); ``out`` may then be None (no bf16 output at all)."""
    ep = Epilogue()
    ep.scale = _p(scale)
    ep.bias = _p(bias)
    ep.act = act
    ep.act_after = act_after
    res = list(residuals) + [None] * (3 - len(residuals))
    ldr = 0
    for r in residuals:
        _need_gpu(r)
        assert r.dtype == BF16 and r.ndim == 2 and r.stride(1) == 1 and r.shape[1] >= N
        ldr = ldr or r.stride(0)
        assert r.stride(0) == ldr, "all residuals must share a row stride"
    ep.res0, ep.res1, ep.res2 = _p(res[0]), _p(res[1]), _p(res[2])
    ep.ldr = ldr
    if out is not None:
        ep.C = out.data_ptr()
        ep.ldc = out.stride(0)
        ep.out_f32 = 1 if out.dtype == torch.float32 else 0
    if mx_out is not None:
        q8, sc8 = mx_out
        _need_gpu(q8, sc8)
        assert q8.dtype == torch.uint8 and q8.ndim == 2 and q8.stride(1) == 1 and q8.shape[0] >= M and q8.stride(0) == ceil_to(N, 128)
        assert sc8.dtype == torch.uint8 and sc8.numel() == int(L.load().mg_mx_scale_bytes(M, N))
        ep.C8, ep.ldc8, ep.c8_scales, ep.c8_rgroups = q8.data_ptr(), q8.stride(0), sc8.data_ptr(), (M + 63) // 64
    if aux is not None and aux_mode != MG_AUX_NONE:
        _need_gpu(aux)
        assert aux.dtype == BF16 and aux.ndim == 2 and aux.stride(1) == 1 and aux.shape[1] >= N
        ep.aux, ep.ldaux, ep.aux_mode, ep.aux_after = aux.data_ptr(), aux.stride(0), aux_mode, int(bool(aux_after))
    if out2 is not None:
        assert out2.dtype == BF16 and out2.ndim == 2 and out2.stride(1) == 1 and out2.shape[1] >= N
        ep.C2, ep.ldc2 = out2.data_ptr(), out2.stride(0)
    return ep


_SPLITK_WS = {}


def splitk_workspace(device) -> torch.Tensor:
    """fp32 scratch of the split-K GEMMs, one per (device, stream) -- launches on one stream are ordered,
    so they can share it.  MAGMA_SPLITK_WS_MB sizes it (default 64)."""
    key = (torch.cuda.current_device(), _stream())        # same device / stream the kernels launch on
    ws = _SPLITK_WS.get(key)
    if ws is None:
        mb = int(os.environ.get("MAGMA_SPLITK_WS_MB", "64"))
        ws = _SPLITK_WS[key] = torch.empty(mb << 18, dtype=torch.float32, device=device)
    return ws


def gemm(a: torch.Tensor, w: PackedLinear, out: Optional[torch.Tensor] = None, *, act: int = MG_ACT_NONE,
         residuals: Sequence[torch.Tensor] = (), act_after: int = MG_ACT_NONE, scale=None,
         use_bias: bool = True, out_dtype=BF16, layout: Optional[str] = None,
         conv: Optional[tuple] = None, aux=None, aux_mode: int = MG_AUX_NONE, aux_after: bool = False,
         out2: Optional[torch.Tensor] = None, tile: int = 0, split_k: int = 0, act_n0: int = 0,
         accumulate: bool = False, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N] = epilogue(a[M,K] @ w^T).  ``act_n0``: ``act`` applies to output columns >= act_n0 only.  ``conv=(H, W, Cin)`` switches the A
    loader to implicit-im2col 3x3 over an NHWC image (a = [B*H*W, Cin]).
    ``split_k``: 0 lets the library cut K when the grid would leave the chip idle, 1 never, n forces n.
    ``accumulate`` (fp32 ``out`` only): out += ... instead of out = ...; ``row_scale`` fp32 [M]: per-row factor of the accumulator
    (mg_epilogue.accumulate / .row_scale -- the weight-gradient GEMMs add into the gradient buffer in place)."""
    _need_gpu(a)
    assert a.dtype == BF16 and a.ndim == 2 and a.stride(1) == 1
    M = a.shape[0]
    if out is None:  # row stride padded to 8 elements (the C ABI wants ldc % 4 == 0)
        out = torch.empty(M, ceil_to(w.N, 8), dtype=out_dtype, device=a.device)[:, : w.N]
    assert out.ndim == 2 and out.shape[0] == M and out.shape[1] >= w.N and out.stride(1) == 1
    d = GemmDesc()
    d.A, d.lda = a.data_ptr(), a.stride(0)
    if layout is None:
        layout = "ft" if w.ft is not None else "rm"
    if layout == "ft":
        d.W, d.ldw, d.w_layout = w.ft.data_ptr(), w.Kp, MG_W_FRAGTILED
    else:
        d.W, d.ldw, d.w_layout = w.rm.data_ptr(), w.rm.stride(0), MG_W_ROWMAJOR
    d.M, d.N, d.K = M, w.N, w.K
    if conv is None:
        assert a.shape[1] == w.K, f"A has K={a.shape[1]}, weight has K={w.K}"
        d.a_mode = MG_A_DENSE
    else:
        d.a_mode = MG_A_CONV3X3
        d.H, d.Wd, d.Cin = conv
        assert a.shape[1] == conv[2] and a.is_contiguous() and w.K == 9 * conv[2]
    d.zero_page = zero_page(a.device).data_ptr()
    d.tile_hint = tile
    d.split_k = split_k
    if split_k != 1:
        ws = splitk_workspace(a.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    d.ep = _epilogue(out, w.N, w.bias if use_bias else None, scale, act, residuals, act_after, aux, aux_mode,
                     aux_after, out2)
    d.ep.act_n0 = act_n0
    if accumulate:
        assert out.dtype == torch.float32, "accumulate adds into an fp32 output"
        d.ep.accumulate = 1
    if row_scale is not None:
        _need_gpu(row_scale)
        assert row_scale.dtype == torch.float32 and row_scale.is_contiguous() and row_scale.numel() >= M
        d.ep.row_scale = row_scale.data_ptr()
    check(L.load().mg_gemm_bf16(C.byref(d), _stream()), "mg_gemm_bf16")
    return out


class RawWeight:
    """Row-major [N, K] bf16 tensor used directly as the GEMM B operand (no copy):
    trainable weights, and the transposed activations of the wgrad GEMMs."""

    def __init__(self, w: torch.Tensor, bias: Optional[torch.Tensor] = None, K: Optional[int] = None):
        _need_gpu(w)
        assert w.dtype == BF16 and w.ndim == 2 and w.stride(1) == 1 and w.stride(0) % 8 == 0
        self.N = w.shape[0]
        self.K = w.shape[1] if K is None else K
        self.Kp = w.stride(0)
        self.rm, self.ft = w, None
        self.bias = bias


def pad_k_rowmajor(w: torch.Tensor) -> torch.Tensor:
    """[N, K] bf16 -> contiguous row-major GEMM operand whose row stride is a multiple of 8 elements."""
    n, k = w.shape
    if k % 8 == 0:
        return w.contiguous()
    out = torch.zeros(n, ceil_to(k, 8), dtype=w.dtype, device=w.device)
    out[:, :k] = w
    return out


def skinny_desc(x: torch.Tensor, w: PackedLinear, out: Optional[torch.Tensor] = None, *, act: int = MG_ACT_NONE,
                residuals: Sequence[torch.Tensor] = (), act_after: int = MG_ACT_NONE, scale=None,
                use_bias: bool = True, out_dtype=BF16, variant: int = 0, ln_fold: Optional[tuple] = None,
                split: Optional[tuple] = None, aux=None, aux_mode: int = MG_AUX_NONE, aux_after: bool = False,
                out2: Optional[torch.Tensor] = None):
    """Build the C descriptor of one decode-shape (M <= 16) weight-streaming GEMM.  Returns
    (desc, out, keepalive).  ``aux`` / ``aux_mode`` / ``aux_after`` / ``out2`` as for ``gemm`` (mg_epilogue.aux / .C2: the GEMV
    then runs the general epilogue instead of its four-column fast path); with ``split`` they belong to the first segment."""
    _need_gpu(x)
    assert x.dtype == BF16 and x.ndim == 2 and x.stride(1) == 1 and w.ft is not None
    assert x.shape[1] == w.Kp, "decode activations must span the padded K"
    w8 = isinstance(w, PackedLinearW8)
    M = x.shape[0]
    if out is None:
        out = torch.empty(M, ceil_to(w.N, 8), dtype=out_dtype, device=x.device)[:, : w.N]
    d = SkinnyDesc()
    d.X, d.ldx, d.W = x.data_ptr(), x.stride(0), w.ft.data_ptr()
    d.M, d.N, d.Kp, d.nt_hint = M, w.N, w.Kp, variant
    if w8:
        d.w_scale = w.scale.data_ptr()
    elif isinstance(w, PackedLinearW4):
        d.w_mx4_scale = w.scales.data_ptr()
    elif DECODE_PACK and getattr(w, "pk", None) is not None:
        pk = w.pk
        d.pk_lo, d.pk_nib, d.pk_base = pk.lo.data_ptr(), pk.nib.data_ptr(), pk.base.data_ptr()
        d.pk_sign, d.pk_flags = pk.sign.data_ptr(), pk.flags.data_ptr()
    n_a = w.N if split is None else split[0]
    d.ep = _epilogue(out, n_a, w.bias if use_bias else None, scale, act, residuals, act_after, aux, aux_mode, aux_after, out2)
    if ln_fold is not None:
        cs, dd, eps = ln_fold
        d.ln_colsum, d.ln_inv_d, d.ln_eps = cs.data_ptr(), 1.0 / dd, eps
    if split is not None:
        split_n, out_b, act_b, bias_b = split
        d.split_n = split_n
        d.ep_b = _epilogue(out_b, w.N - split_n, bias_b, None, act_b, (), MG_ACT_NONE)
    return d, out


class PackedLinearW8:
    """Decode weight as e4m3 bytes + one fp32 scale per output channel, for the W8A16 weight-streaming GEMV (bf16
    activations; the kernel widens the bytes in registers).  ``ft`` = [ceil(N/16)][Kp/64][64 lanes][16 B]: lane
    kq*16+n holds W[n][64j + 8kq .. +7] then W[n][64j + 32 + 8kq .. +7].  K must be a multiple of 1024."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None):
        _need_gpu(weight)
        self.N, self.K = weight.shape
        assert self.K % 1024 == 0, "W8A16 decode weights need K % 1024 == 0"
        self.Kp = self.K
        n16 = ceil_to(self.N, 16)
        w = torch.zeros(n16, self.K, dtype=BF16, device=weight.device)
        w[: self.N] = weight.detach().to(BF16)
        q, sc = quantize_rows_fp8(w, self.K)
        self.scale = sc.contiguous()                               # padded to n16 (rows beyond N are zero)
        self.bias = None if bias is None else bias.detach().to(torch.float32).contiguous()
        # [n16, K] -> [nt, n(16), pair j, step(2), kq(4), 8] -> [nt, j, kq, n, step, 8]
        self.ft = q.view(n16 // 16, 16, self.K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).contiguous()

    def dequant(self) -> torch.Tensor:
        n16 = self.ft.shape[0] * 16
        q = self.ft.permute(0, 3, 1, 4, 2, 5).reshape(n16, self.K)
        return (q.view(torch.float8_e4m3fn).float() * self.scale[:, None])[: self.N]


_E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_E2M1_MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def quantize_mx_fp4(w: torch.Tensor):
    """[N, K] (K % 32 == 0) -> (codes uint8 [N, K/2], scales uint8 [N, K/32]): OCP MX v1.0 MXFP4.  Per 32 consecutive K-elements
    of a row the shared exponent is e = floor(log2 amax) - 2 (2 = the exponent of e2m1's largest value, 6), clamped to
    [-125, 124] so that every non-zero dequantised value is a NORMAL bf16 and ``scale_byte << 23`` is the fp32 scale; the
    elements are w * 2^-e rounded to nearest, ties to the even code, onto +-{0, .5, 1, 1.5, 2, 3, 4, 6}, saturating at +-6.  An
    all-zero block has all-zero codes (scale byte 127); a value that rounds to zero is stored as +0.  Element 2i sits in the
    low nibble of byte i.  Plain torch on any device."""
    assert w.ndim == 2 and w.shape[1] % 32 == 0, "MXFP4 blocks are 32 K-elements"
    N, K = w.shape
    blk = w.detach().to(torch.float32).reshape(N, K // 32, 32)
    amax = blk.abs().amax(-1)
    _, ex = torch.frexp(amax)                                   # amax = m * 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e = torch.where(amax > 0, ex - 3, torch.zeros_like(ex)).clamp(-125, 124)
    a = torch.ldexp(blk, -e[..., None]).abs()                   # exact: a power-of-two factor
    mag = torch.zeros(a.shape, dtype=torch.uint8, device=w.device)
    for j, m in enumerate(_E2M1_MIDPOINTS):                     # code j | j+1 meet at m: the tie goes to the even one
        mag += (a >= m) if j & 1 else (a > m)
    code = mag | (((blk < 0) & (mag > 0)).to(torch.uint8) << 3)
    code = code.reshape(N, K // 2, 2)
    return (code[..., 0] | (code[..., 1] << 4)).contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequantize_mx_fp4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """(codes [N, K/2], scales [N, K/32]) -> the exact fp32 values [N, K] (each one is also a bf16 value)."""
    N, K = codes.shape[0], codes.shape[1] * 2
    c = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(N, K).long()
    v = torch.tensor(_E2M1_VALUES, dtype=torch.float32, device=codes.device)[c & 7]
    v = torch.where((c & 8) != 0, -v, v)
    e = (scales.to(torch.int32) - 127).repeat_interleave(32, dim=1)
    return torch.ldexp(v, e)


def tile_mx_fp4(codes: torch.Tensor, scales: torch.Tensor):
    """Row-major MXFP4 (quantize_mx_fp4; K % 128 == 0) -> the W4A16 GEMV's operands, rows zero-padded to a multiple of 16:
    codes  [ceil(N/16)][K/128][64 lanes][16 B], lane = kq*16 + n, bytes 4s..4s+3 = the codes of W[n][128j + 32s + 8kq .. +7];
    scales [ceil(N/16)][K/128][16 n][4 B], byte s = the E8M0 scale of W[n][128j + 32s .. +31] (padding rows: 127)."""
    N, K = codes.shape[0], codes.shape[1] * 2
    assert K % 128 == 0 and scales.shape == (N, K // 32)
    n16 = ceil_to(N, 16)
    c = torch.zeros(n16, K // 2, dtype=torch.uint8, device=codes.device)
    c[:N] = codes
    sc = torch.full((n16, K // 32), 127, dtype=torch.uint8, device=codes.device)
    sc[:N] = scales
    # [n16, K/2] -> [nt, n(16), quad j, step s(4), kq(4), 4 B] -> [nt, j, kq, n, s, 4 B]
    ft = c.view(n16 // 16, 16, K // 128, 4, 4, 4).permute(0, 2, 4, 1, 3, 5).contiguous()
    st = sc.view(n16 // 16, 16, K // 128, 4).permute(0, 2, 1, 3).contiguous()
    return ft, st


def untile_mx_fp4(ft: torch.Tensor, st: torch.Tensor, N: int):
    """Inverse of tile_mx_fp4: row-major (codes [N, K/2], scales [N, K/32])."""
    nt, kq4 = ft.shape[0], ft.shape[1]
    codes = ft.permute(0, 3, 1, 4, 2, 5).reshape(nt * 16, kq4 * 64)
    scales = st.permute(0, 2, 1, 3).reshape(nt * 16, kq4 * 4)
    return codes[:N].contiguous(), scales[:N].contiguous()


class PackedLinearW4:
    """Decode weight as OCP MXFP4 (e2m1 codes + one E8M0 scale per 32 K-elements, 4.25 bits per weight) for the W4A16
    weight-streaming GEMV (bf16 activations; the kernel widens the codes in registers with the block scale applied, exactly).
    ``ft`` / ``scales``: the tiled codes and scale bytes (tile_mx_fp4; include/magma_hip.h mg_skinny_desc.w_mx4_scale).  K must
    be a multiple of 512: four waves split K, each in whole k-step quads (one 16-byte lane load = 4 k-steps = 128 K-elements).
    Packing is plain torch: it runs on the weight's device, the CPU included."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None):
        self.N, self.K = weight.shape
        assert self.K % 512 == 0, "W4A16 decode weights need K % 512 == 0"
        self.Kp = self.K
        self.ft, self.scales = tile_mx_fp4(*quantize_mx_fp4(weight))
        self.bias = None if bias is None else bias.detach().to(torch.float32).contiguous()

    def dequant(self) -> torch.Tensor:
        """The exact fp32 values [N, K] the kernel multiplies (every one a bf16 value)."""
        return dequantize_mx_fp4(*untile_mx_fp4(self.ft, self.scales, self.N))


DECODE_PACK = True      # skinny_desc hands a PackedLinear's lossless twin (.pk, attach_decode_pack) to the kernel; False: never


def pack_bf16_lossless(w: torch.Tensor):
    """Row-major bf16 [n16, K] (n16 % 16 == 0, K % 128 == 0) -> (lo, nib, base, sign, flags): the same bits in 13.25 per weight, in
    the lane layouts of the packed weight-streaming GEMV (include/magma_hip.h, mg_skinny_desc.pk_lo).  A bf16 is s | e[7:0] | m[6:0]:
    the low byte e0<<7 | m goes to ``lo`` verbatim, the high byte is the sign (``sign``) and eh = e>>1, stored as the 4-bit offset
    eh - base (``nib``) against base = min(eh) over the 32 K-elements of a row that one MFMA k-step consumes (``base``, one byte per
    block).  A block whose eh span exceeds 15 does not fit: its 16-row tile is flagged in ``flags`` (uint8, padded with zeros to a
    multiple of 16 entries) and its planes hold clamped offsets nobody reads for values.  Plain torch on the weight's device."""
    assert w.dtype == BF16 and w.ndim == 2 and w.shape[0] % 16 == 0 and w.shape[1] % 128 == 0
    n16, K = w.shape
    nt, kq4 = n16 // 16, K // 128
    bits = w.contiguous().view(torch.int16)
    lowb = (bits & 0xff).to(torch.uint8)
    high = ((bits >> 8) & 0xff).to(torch.uint8)
    del bits
    eh = high & 0x7f
    blk = eh.view(n16, K // 32, 32)
    base = blk.amin(-1)
    misfit = (blk.amax(-1) - base) > 15                                  # uint8 arithmetic: amax >= base
    flags = torch.zeros(ceil_to(nt, 16), dtype=torch.uint8, device=w.device)
    flags[:nt] = misfit.view(nt, 16, K // 32).any(2).any(1).to(torch.uint8)
    off = (blk - base[..., None]).clamp_(max=15).view(n16, K)
    # [n16, K] -> [nt, n(16), pair, step(2), kq(4), 8] -> [nt, pair, kq, n, step, 8]  (PackedLinearW8.ft's lane layout)
    lo = lowb.view(nt, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).contiguous()
    # element 8kq + 4g + b of k-step 4j + s: [nt, n, j, s, kq, g, b]
    o7 = off.view(nt, 16, kq4, 4, 4, 2, 4)
    nib = (o7[..., 0, :] | (o7[..., 1, :] << 4)).permute(0, 2, 4, 1, 3, 5).contiguous()       # [nt, j, kq, n, s, b]
    base_t = base.view(nt, 16, kq4, 4).permute(0, 2, 1, 3).contiguous().view(torch.int32).squeeze(-1)     # [nt, j, n] words
    # sign of (s, g, b) at bit 8b + 7 - (2s + g): byte b of the word collects the eight (s, g) of its column
    sh = (7 - (2 * torch.arange(4, device=w.device)[:, None] + torch.arange(2, device=w.device)[None, :])).to(torch.uint8)
    s7 = (high >> 7).view(nt, 16, kq4, 4, 4, 2, 4) << sh[:, None, :, None]                       # [.., s, kq, g, b]
    sign = s7.sum(dim=(3, 5), dtype=torch.uint8).permute(0, 2, 3, 1, 4).contiguous().view(torch.int32).squeeze(-1)   # [nt, j, kq, n]
    return lo, nib, base_t, sign, flags


def unpack_bf16_lossless(lo: torch.Tensor, nib: torch.Tensor, base: torch.Tensor, sign: torch.Tensor) -> torch.Tensor:
    """Exact inverse of pack_bf16_lossless over the tiles that are not flagged: the row-major bf16 [n16, K] the kernel rebuilds."""
    nt, kq4 = nib.shape[0], nib.shape[1]
    n16, K = nt * 16, kq4 * 128
    lowb = lo.permute(0, 3, 1, 4, 2, 5).reshape(n16, K).to(torch.int32)
    nb = nib.permute(0, 3, 1, 4, 2, 5)                                                            # [nt, n, j, s, kq, b]
    off = torch.stack([nb & 15, nb >> 4], dim=5).reshape(n16, K).to(torch.int32)                  # [nt, n, j, s, kq, g, b]
    bs = base.contiguous().view(nt, kq4, 16, 1).view(torch.uint8).permute(0, 2, 1, 3).reshape(n16, K // 32)   # [nt, n, j, s]
    sg = sign.contiguous().view(nt, kq4, 4, 16, 1).view(torch.uint8).permute(0, 3, 1, 2, 4)        # [nt, n, j, kq, b]
    dev = lo.device
    sh = (7 - (2 * torch.arange(4, device=dev)[:, None] + torch.arange(2, device=dev)[None, :])).to(torch.uint8)   # [s, g]
    s7 = (sg[:, :, :, None, :, None, :] >> sh[:, None, :, None]) & 1                               # [nt, n, j, s, kq, g, b]
    high = (s7.reshape(n16, K).to(torch.int32) << 7) | (off + bs.to(torch.int32).repeat_interleave(32, dim=1))
    return ((high << 8) | lowb).to(torch.int16).view(BF16)


class DecodePack:
    """The lossless 13.25-bit twin of a fragment-tiled bf16 PackedLinear (pack_bf16_lossless): what the decode GEMVs stream instead
    of ``ft`` -- same bits out, 0.83x the bytes in.  The bf16 operand stays: the workgroups of flagged row tiles read it."""

    def __init__(self, ft: torch.Tensor):
        self.lo, self.nib, self.base, self.sign, self.flags = pack_bf16_lossless(PackedLinear.untile(ft))
        self.ntiles = ft.shape[0]
        self.escaped = int(self.flags.count_nonzero())

    def unpack(self) -> torch.Tensor:
        return unpack_bf16_lossless(self.lo, self.nib, self.base, self.sign)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.lo, self.nib, self.base, self.sign, self.flags))


def attach_decode_pack(w: PackedLinear) -> Optional[DecodePack]:
    """Give a bf16 PackedLinear its lossless twin as ``w.pk`` (skinny_desc then fills mg_skinny_desc.pk_*); an operand the packed
    kernels do not take (Kp not a multiple of 512: four waves in whole k-step quads; not a plain PackedLinear) gets none."""
    if type(w) is not PackedLinear or w.ft is None or w.Kp % 512:
        return None
    if getattr(w, "pk", None) is None:
        w.pk = DecodePack(w.ft)
    return w.pk


def gemm_skinny(x: torch.Tensor, w: PackedLinear, out: Optional[torch.Tensor] = None, **kw) -> torch.Tensor:
    """Decode-shape (M <= 16) weight-streaming GEMM; needs the fragment-tiled layout.
    ``ln_fold=(colsum fp32 [N], d, eps)``: LayerNorm of x folded into the GEMV (weights and
    bias must be pre-folded, see fold_layernorm).  ``split=(split_n, out_b, act_b, bias_b)``:
    columns >= split_n are written to ``out_b`` with their own activation / bias vector."""
    d, out = skinny_desc(x, w, out, **kw)
    check(L.load().mg_gemm_skinny_bf16(C.byref(d), _stream()), "mg_gemm_skinny_bf16")
    return out


def gemm_skinny2(a: tuple, b: tuple):
    """Two independent decode GEMVs in one launch; a, b = (x, w, out, kwargs)."""
    da, oa = skinny_desc(a[0], a[1], a[2], **a[3])
    db, ob = skinny_desc(b[0], b[1], b[2], **b[3])
    check(L.load().mg_gemm_skinny2_bf16(C.byref(da), C.byref(db), _stream()), "mg_gemm_skinny2_bf16")
    return oa, ob


def _pos_stride(d_pos: torch.Tensor, B: int, pos_stride: int) -> int:
    """pos_stride 0: one write position shared by the batch (d_pos[0]); 1: row b at d_pos[b] (ragged batches)."""
    assert d_pos.dtype == torch.int32 and d_pos.is_contiguous()
    if pos_stride not in (0, 1):
        raise ValueError("pos_stride must be 0 (one shared position) or 1 (one position per row)")
    if pos_stride == 1 and d_pos.numel() < B:
        raise ValueError(f"pos_stride=1 needs one position per row: d_pos has {d_pos.numel()} entries for B = {B}")
    return pos_stride


def decode_attn_gemv(qkv, kcache, vcache, attn_out, B, H, d_pos, rot_dim, sin_t, cos_t, gemv: tuple, *, pos_stride: int = 0,
                     shared=None, chunk: int = 0):
    """Decode attention (rotary + append + attend) co-launched with one independent GEMV
    gemv = (x, w, out, kwargs).  ``pos_stride=1``: row b writes / attends at its own position d_pos[b].
    ``shared`` = (n_prefix, part): the attention runs in the shared-prefix mode (attn_decode_fused) -- another entry point.
    ``chunk`` = T >= 2 (mg_decode_attn_gemv_chunk_bf16, one launch as well): ``qkv`` / ``attn_out`` hold B * T rows, T consecutive
    positions of each of the B sequences -- the attention workgroups run attn_decode_chunk's body --, the GEMV runs over its
    M = B * T operand with the bits of the plain co-launch's."""
    _need_gpu(qkv)
    ps = _pos_stride(d_pos, B, pos_stride)
    d, og = skinny_desc(gemv[0], gemv[1], gemv[2], **gemv[3])
    assert attn_out.ndim == 2 and attn_out.stride(1) == 1 and attn_out.shape[1] == H * 256   # a column range of a wider row is fine
    if chunk:
        assert shared is None
        check(L.load().mg_decode_attn_gemv_chunk_bf16(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), attn_out.data_ptr(),
                                                      attn_out.stride(0), B, int(chunk), H, kcache.shape[2], d_pos.data_ptr(), rot_dim,
                                                      _p(sin_t), _p(cos_t), C.byref(d), ps, _stream()),
              "mg_decode_attn_gemv_chunk_bf16")
        return attn_out, og
    if shared is not None:
        n_prefix, part = _shared_part(shared, B, H)
        check(L.load().mg_decode_attn_gemv_shared_bf16(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), attn_out.data_ptr(),
                                                       attn_out.stride(0), B, H, kcache.shape[2], d_pos.data_ptr(), rot_dim,
                                                       sin_t.data_ptr(), cos_t.data_ptr(), C.byref(d), ps, n_prefix, part.data_ptr(),
                                                       _stream()), "mg_decode_attn_gemv_shared_bf16")
        return attn_out, og
    check(L.load().mg_decode_attn_gemv_bf16(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), attn_out.data_ptr(),
                                            attn_out.stride(0), B, H, kcache.shape[2], d_pos.data_ptr(), rot_dim, sin_t.data_ptr(),
                                            cos_t.data_ptr(), C.byref(d), ps, _stream()), "mg_decode_attn_gemv_bf16")
    return attn_out, og


def fold_layernorm(weight: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """LN(x) W^T + b  ==  rstd*(x W'^T - mean*colsum) + b'  with  W' = W*gamma (bf16),
    colsum[n] = sum_k W'[n][k] (of the rounded W'), b' = b + W beta.  One-off weight prep."""
    wf = weight.detach().float()
    w2 = (wf * gamma.float()[None, :]).to(BF16)
    colsum = w2.float().sum(1).contiguous()
    b2 = wf @ beta.float()
    if bias is not None:
        b2 = b2 + bias.detach().float()
    return w2, b2.contiguous(), colsum


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _need_gpu(x)
    assert x.dtype == BF16 and x.ndim == 2 and x.stride(1) == 1
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    check(L.load().mg_layernorm_bf16(x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(),
                                     out.data_ptr(), out.stride(0), x.shape[0], x.shape[1], eps, _stream()),
          "mg_layernorm_bf16")
    return out


def embedding(ids: torch.Tensor, wte: torch.Tensor, out: torch.Tensor, row_off: int = 0) -> torch.Tensor:
    """out[b, row_off + t, :] = wte[ids[b, t]]; out is (B, S_total, d) contiguous.

    An id outside [0, vocab) is CLAMPED, silently and without a device sync: a negative id reads row 0, an id >= vocab reads row
    vocab - 1; nothing outside ``wte`` is ever read (tests/test_row_kernels_gpu.py pins it).  The loss path does not share that
    leniency: cross_entropy ignores such a target, and the engines refuse it where the labels are on the host."""
    _need_gpu(ids, wte, out)
    assert ids.dtype == torch.int64 and ids.ndim == 2 and ids.is_contiguous()
    assert wte.dtype == BF16 and wte.is_contiguous() and out.dtype == BF16 and out.ndim == 3
    B, T = ids.shape
    assert out.stride(2) == 1 and out.stride(1) == out.shape[2] and row_off + T <= out.shape[1]
    check(L.load().mg_embedding_bf16(ids.data_ptr(), B, T, wte.data_ptr(), wte.shape[0], wte.shape[1],
                                     out.data_ptr(), out.stride(0), row_off, _stream()), "mg_embedding_bf16")
    return out


def rotary_split(qkv, B, S, H, rot_dim, sin_t, cos_t, q_out, kcache, vcache, *, pos0: int = 0,
                 d_pos: Optional[torch.Tensor] = None, vt: Optional[torch.Tensor] = None, pos_stride: int = 0):
    """``pos_stride=1`` (with ``d_pos`` of B positions, no ``vt``): row b's S rows land at d_pos[b] + s -- a chunk appended to a
    ragged cache (slots at or past Smax are skipped)."""
    _need_gpu(qkv)
    assert qkv.ndim == 2 and qkv.stride(1) == 1          # [B*S, >= 3*H*256]: a column range of a wider GEMM output is fine
    Smax = kcache.shape[2]
    ps = 0
    if pos_stride:
        if d_pos is None or vt is not None:
            raise ValueError("rotary_split(pos_stride=1) needs d_pos and no vt")
        ps = _pos_stride(d_pos, B, pos_stride)
    check(L.load().mg_rotary_split_bf16(qkv.data_ptr(), qkv.stride(0), B, S, H, rot_dim, sin_t.data_ptr(), cos_t.data_ptr(), pos0,
                                        _p(d_pos), q_out.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), Smax,
                                        _p(vt), 0 if vt is None else vt.shape[2] * 32, ps, _stream()),
          "mg_rotary_split_bf16")


def rotary_split_train(qkv, B, S, H, rot_dim, sin_t, cos_t, q, k, v, vt, qt, kt):
    """Training form of rotary_split: q, k, v [B,H,S,256] and the three transposes [B,H,ld/32,256,32] in one pass."""
    _need_gpu(qkv)
    check(L.load().mg_rotary_split_train_bf16(qkv.data_ptr(), B, S, H, rot_dim, sin_t.data_ptr(), cos_t.data_ptr(),
                                              q.data_ptr(), k.data_ptr(), v.data_ptr(), vt.data_ptr(), qt.data_ptr(),
                                              kt.data_ptr(), vt.shape[2] * 32, _stream()), "mg_rotary_split_train_bf16")


class AttnFP8Operands:
    """What mg_rotary_split_fp8 writes for the fp8 attention forward (include/magma_hip.h): OCP MX e4m3 copies of the rotated q, k
    and of v^T with their E8M0 scales."""

    def __init__(self, B, H, S, device):
        self.B, self.H, self.S = B, H, S
        self.Sp = int(L.load().mg_attn_fp8_scale_stride(S))
        nt = (S + 63) // 64
        u8 = dict(dtype=torch.uint8, device=device)
        self.q8, self.k8 = torch.empty(B, H, S, 256, **u8), torch.empty(B, H, S, 256, **u8)
        self.v8t = torch.empty(B, H, nt, 256, 64, **u8)
        self.eq, self.ek = torch.full((B, H, self.Sp), 127, **u8), torch.full((B, H, self.Sp), 127, **u8)
        self.sv8 = torch.empty(B, H, nt, 512, **u8)

    def dequant(self):
        """(q, k, v) [B,H,S,256] fp32: the values the fp8 attention kernel multiplies (tests / oracles)."""
        B, H, S = self.B, self.H, self.S
        f8 = torch.float8_e4m3fn
        sq = torch.exp2(self.eq[:, :, :S].float() - 127.0)[..., None]
        sk = torch.exp2(self.ek[:, :, :S].float() - 127.0)[..., None]
        q = self.q8.view(f8).float() * sq
        k = self.k8.view(f8).float() * sk
        nt = self.v8t.shape[2]
        vt = self.v8t.view(f8).float()                                     # [B,H,nt,256 d,64 bytes]
        sv = torch.exp2(self.sv8.view(B, H, nt, 2, 32, 8).float() - 127.0)  # [key block][d % 32][d / 32]
        sv = sv.permute(0, 1, 2, 3, 5, 4).reshape(B, H, nt, 2, 256)        # -> [key block][d]
        # byte 32 hi + 16 b + r  <->  key 32 b + (r & 3) + 8 (r >> 2) + 4 hi
        idx = torch.empty(64, dtype=torch.long)
        blk = torch.empty(64, dtype=torch.long)
        for hi in range(2):
            for b in range(2):
                for r in range(16):
                    idx[32 * b + (r & 3) + 8 * (r >> 2) + 4 * hi] = 32 * hi + 16 * b + r
                    blk[32 * b + (r & 3) + 8 * (r >> 2) + 4 * hi] = b
        idx, blk = idx.to(vt.device), blk.to(vt.device)
        v_keys = vt[..., idx]                                              # [B,H,nt,256,64 keys in natural order]
        v_keys = v_keys * sv[:, :, :, blk, :].permute(0, 1, 2, 4, 3)        # scale of (key block, d)
        v = v_keys.permute(0, 1, 2, 4, 3).reshape(B, H, nt * 64, 256)[:, :, :S]
        return q, k, v


def rotary_split_fp8(qkv, B, S, H, rot_dim, sin_t, cos_t, q=None, k=None, v=None, qt=None, kt=None, inplace: bool = False) -> AttnFP8Operands:
    """rotary_split_train without V^T + the OCP MX e4m3 operands of the fp8 attention forward (-> AttnFP8Operands).
    q / k / v (and qt / kt) None: forward only, just the e4m3 operands.  ``inplace``: the rotated q / k are also written back into
    ``qkv`` (rotary_qk_inplace's result from this pass)."""
    _need_gpu(qkv)
    assert qkv.is_contiguous() and qkv.shape == (B * S, 3 * H * 256)
    op = AttnFP8Operands(B, H, S, qkv.device)
    check(L.load().mg_rotary_split_fp8(qkv.data_ptr(), B, S, H, rot_dim, sin_t.data_ptr(), cos_t.data_ptr(), _p(q), _p(k),
                                       _p(v), _p(qt), _p(kt), (qt.shape[2] * 32) if qt is not None else 0,
                                       op.q8.data_ptr(), op.k8.data_ptr(), op.v8t.data_ptr(), op.eq.data_ptr(), op.ek.data_ptr(),
                                       op.sv8.data_ptr(), int(bool(inplace)), _stream()), "mg_rotary_split_fp8")
    return op


def attn_prefill_fp8(op: AttnFP8Operands, out, lse: Optional[torch.Tensor] = None, mx_out=None):
    """Causal flash attention on the fp8 MFMA (mg_attn_prefill_fp8): out [B*S, >= H*256] bf16 (a column range of a wider row is fine).
    ``mx_out`` = (q, scales) from mx_empty(B*S, H*256): the epilogue also writes the OCP MX e4m3 copy of out."""
    assert out.ndim == 2 and out.stride(1) == 1 and out.shape[1] == op.H * 256 and out.stride(0) % 8 == 0
    q8, sc8 = mx_out if mx_out is not None else (None, None)
    if q8 is not None:
        assert q8.dtype == torch.uint8 and q8.shape[0] >= op.B * op.S and q8.stride(0) == ceil_to(op.H * 256, 128)
        assert sc8.numel() == int(L.load().mg_mx_scale_bytes(op.B * op.S, op.H * 256))
    check(L.load().mg_attn_prefill_fp8(op.q8.data_ptr(), op.k8.data_ptr(), op.v8t.data_ptr(), op.eq.data_ptr(), op.ek.data_ptr(),
                                       op.sv8.data_ptr(), out.data_ptr(), out.stride(0), _p(lse), op.B, op.H, op.S,
                                       _p(q8), 0 if q8 is None else q8.stride(0), _p(sc8), _stream()),
          "mg_attn_prefill_fp8")
    return out


def attn_prefill(q, kcache, vt, out, B, H, S, lse: Optional[torch.Tensor] = None):
    _need_gpu(q)
    assert out.ndim == 2 and out.stride(1) == 1 and out.shape[1] == H * 256      # a column range of a wider row is fine
    check(L.load().mg_attn_prefill_bf16(q.data_ptr(), kcache.data_ptr(), vt.data_ptr(), out.data_ptr(), out.stride(0), _p(lse),
                                        B, H, S, kcache.shape[2], vt.shape[2] * 32, _stream()), "mg_attn_prefill_bf16")
    return out


def attn_prefill_scaled(q, kcache, vt, out, B, H, S, key_scale, lse: Optional[torch.Tensor] = None):
    """attn_prefill with every score multiplied by its key's scale before the causal mask (mg_attn_prefill_scaled_bf16; DESIGN.md
    "Explaining an answer"): s[t, j] = (q_t . k_j) / 16 * key_scale[b, j] in fp32.  ``key_scale`` fp32 (B, >= S) with unit column
    stride (row stride = its stride(0); the heads of a row share it); entries finite and >= 0 -- the callers' duty (LMEngine.score
    checks on the host), the kernel does not look.  The other operands are attn_prefill's; S <= 4096."""
    _need_gpu(q, key_scale)
    if q.ndim != 4 or tuple(q.shape) != (B, H, S, 256) or not q.is_contiguous() or q.dtype != torch.bfloat16:
        raise ValueError(f"q must be a contiguous bf16 ({B}, {H}, {S}, 256) tensor, got {q.dtype} {tuple(q.shape)}")
    if kcache.ndim != 4 or kcache.shape[0] != B or kcache.shape[1] != H or kcache.shape[3] != 256 or not kcache.is_contiguous() \
            or kcache.dtype != torch.bfloat16 or kcache.shape[2] < S:
        raise ValueError(f"kcache must be a contiguous bf16 ({B}, {H}, Smax >= {S}, 256) cache, got {kcache.dtype} {tuple(kcache.shape)}")
    if vt.ndim != 5 or vt.shape[0] != B or vt.shape[1] != H or tuple(vt.shape[3:]) != (256, 32) or not vt.is_contiguous() \
            or vt.dtype != torch.bfloat16 or vt.shape[2] * 32 < S:
        raise ValueError(f"vt must be a contiguous bf16 ({B}, {H}, >= {ceil_to(S, 32) // 32}, 256, 32) tensor, got {vt.dtype} {tuple(vt.shape)}")
    if out.ndim != 2 or out.stride(1) != 1 or out.shape[0] != B * S or out.shape[1] != H * 256 or out.dtype != torch.bfloat16:
        raise ValueError(f"out must be bf16 ({B * S}, {H * 256}) with unit column stride, got {out.dtype} {tuple(out.shape)}")
    if key_scale.dtype != torch.float32 or key_scale.ndim != 2 or key_scale.shape[0] != B or key_scale.shape[1] < S \
            or key_scale.stride(1) != 1 or (B > 1 and key_scale.stride(0) < S):
        raise ValueError(f"key_scale must be fp32 ({B}, >= {S}) with unit column stride, got {key_scale.dtype} {tuple(key_scale.shape)}")
    if lse is not None and (lse.dtype != torch.float32 or lse.numel() != B * H * S or not lse.is_contiguous()):
        raise ValueError(f"lse must be a contiguous fp32 tensor of {B * H * S} elements, got {lse.dtype} {tuple(lse.shape)}")
    check(L.load().mg_attn_prefill_scaled_bf16(q.data_ptr(), kcache.data_ptr(), vt.data_ptr(), out.data_ptr(), out.stride(0), _p(lse),
                                               B, H, S, kcache.shape[2], vt.shape[2] * 32, key_scale.data_ptr(),
                                               key_scale.stride(0) if B > 1 else max(key_scale.stride(0), S), _stream()),
          "mg_attn_prefill_scaled_bf16")
    return out


def attn_prefill_cached(q, kcache, vcache, out, B, H, T, d_pos, *, pos_stride: int = 0):
    """Causal attention of a chunk of T new (already rotated) queries per row against the KV cache: query t of row b sits at
    p_b + t (p_b = d_pos[b * pos_stride]) and sees cache keys [0, p_b + t]; the chunk's K / V must already be in the cache
    (rotary_split with pos_stride).  q [B,H,T,256] (any row / head / batch strides that are multiples of 8, rows contiguous);
    out [B*T, H*256] (a column range of a wider row is fine)."""
    _need_gpu(q)
    if q.ndim != 4 or tuple(q.shape) != (B, H, T, 256) or q.stride(3) != 1 or q.dtype != torch.bfloat16:
        raise ValueError(f"q must be bf16 ({B}, {H}, {T}, 256) with contiguous rows, got {q.dtype} {tuple(q.shape)}")
    for name, c in (("kcache", kcache), ("vcache", vcache)):
        if c.ndim != 4 or c.shape[0] != B or c.shape[1] != H or c.shape[3] != 256 or not c.is_contiguous() or c.dtype != torch.bfloat16:
            raise ValueError(f"{name} must be a contiguous bf16 ({B}, {H}, Smax, 256) cache, got {c.dtype} {tuple(c.shape)}")
    if kcache.shape != vcache.shape:
        raise ValueError("kcache and vcache must have the same shape")
    if out.ndim != 2 or out.stride(1) != 1 or out.shape[0] != B * T or out.shape[1] != H * 256 or out.dtype != torch.bfloat16:
        raise ValueError(f"out must be bf16 ({B * T}, {H * 256}) with unit column stride, got {out.dtype} {tuple(out.shape)}")
    if T > kcache.shape[2]:
        raise ValueError(f"a chunk of {T} rows does not fit a cache of Smax = {kcache.shape[2]}")
    ps = _pos_stride(d_pos, B, pos_stride)
    check(L.load().mg_attn_prefill_cached_bf16(q.data_ptr(), q.stride(2), q.stride(0), q.stride(1), kcache.data_ptr(),
                                               vcache.data_ptr(), out.data_ptr(), out.stride(0), B, H, T, kcache.shape[2],
                                               d_pos.data_ptr(), ps, _stream()), "mg_attn_prefill_cached_bf16")
    return out


def attn_prefill_tree(q, kcache, vcache, out, B, H, T, d_pos, sub, *, p_min: int, pos_stride: int = 0):
    """attn_prefill_cached over a chunk whose T rows are the nodes of a trie in depth-first preorder (DESIGN.md "Ranking choices";
    sampling.trie_rows): ``sub`` int32 (B, T), sub[b, j] = one past the last row of node j's subtree.  Query t of row b sees the
    cache keys [0, p_b) and chunk key j (slot p_b + j) iff j <= t < sub[b, j].  sub == T everywhere is a chain: the bytes of
    attn_prefill_cached.  ``p_min``: the caller's host copy of the smallest p_b -- every query needs a cached key, p_min < 1 is
    refused by the library before the launch.  The other operands are attn_prefill_cached's."""
    _need_gpu(q, sub)
    if q.ndim != 4 or tuple(q.shape) != (B, H, T, 256) or q.stride(3) != 1 or q.dtype != torch.bfloat16:
        raise ValueError(f"q must be bf16 ({B}, {H}, {T}, 256) with contiguous rows, got {q.dtype} {tuple(q.shape)}")
    for name, c in (("kcache", kcache), ("vcache", vcache)):
        if c.ndim != 4 or c.shape[0] != B or c.shape[1] != H or c.shape[3] != 256 or not c.is_contiguous() or c.dtype != torch.bfloat16:
            raise ValueError(f"{name} must be a contiguous bf16 ({B}, {H}, Smax, 256) cache, got {c.dtype} {tuple(c.shape)}")
    if kcache.shape != vcache.shape:
        raise ValueError("kcache and vcache must have the same shape")
    if out.ndim != 2 or out.stride(1) != 1 or out.shape[0] != B * T or out.shape[1] != H * 256 or out.dtype != torch.bfloat16:
        raise ValueError(f"out must be bf16 ({B * T}, {H * 256}) with unit column stride, got {out.dtype} {tuple(out.shape)}")
    if T > kcache.shape[2]:
        raise ValueError(f"a chunk of {T} rows does not fit a cache of Smax = {kcache.shape[2]}")
    if sub is not None and (sub.dtype != torch.int32 or tuple(sub.shape) != (B, T) or not sub.is_contiguous()):
        raise ValueError(f"sub must be a contiguous int32 ({B}, {T}) tensor, got {sub.dtype} {tuple(sub.shape)}")
    ps = _pos_stride(d_pos, B, pos_stride)
    check(L.load().mg_attn_prefill_tree_bf16(q.data_ptr(), q.stride(2), q.stride(0), q.stride(1), kcache.data_ptr(),
                                             vcache.data_ptr(), out.data_ptr(), out.stride(0), B, H, T, kcache.shape[2],
                                             d_pos.data_ptr(), ps, _p(sub), int(p_min), _stream()), "mg_attn_prefill_tree_bf16")
    return out


def rotary_split_at(qkv, B, S, H, rot_dim, sin_t, cos_t, q_out, kcache, vcache, d_pos, off):
    """rotary_split(pos_stride=1) with the slot and the angle apart: row s of sequence b lands in cache slot d_pos[b] + s, rotated
    with the angles of position d_pos[b] + off[b, s] (``off`` int32 (B, S): a trie node's depth - 1).  Slots or positions at or
    past Smax are skipped.  off[b, s] == s gives the bytes of rotary_split(pos_stride=1)."""
    _need_gpu(qkv, d_pos, off)
    assert qkv.ndim == 2 and qkv.stride(1) == 1
    assert d_pos.dtype == torch.int32 and d_pos.is_contiguous() and d_pos.numel() >= B
    if off.dtype != torch.int32 or tuple(off.shape) != (B, S) or not off.is_contiguous():
        raise ValueError(f"off must be a contiguous int32 ({B}, {S}) tensor, got {off.dtype} {tuple(off.shape)}")
    if sin_t.shape[0] < kcache.shape[2]:
        raise ValueError(f"the rotary tables hold {sin_t.shape[0]} positions, the cache {kcache.shape[2]}")
    check(L.load().mg_rotary_split_at_bf16(qkv.data_ptr(), qkv.stride(0), B, S, H, rot_dim, sin_t.data_ptr(), cos_t.data_ptr(),
                                           d_pos.data_ptr(), off.data_ptr(), q_out.data_ptr(), kcache.data_ptr(),
                                           vcache.data_ptr(), kcache.shape[2], _stream()), "mg_rotary_split_at_bf16")


def attn_decode(q, kcache, vcache, out, B, H, d_pos, *, pos_stride: int = 0):
    """Attention of one (already rotated) query per (b, h) over [0, pos_b]; pos_b = d_pos[b * pos_stride]."""
    _need_gpu(q)
    ps = _pos_stride(d_pos, B, pos_stride)
    check(L.load().mg_attn_decode_bf16(q.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), B, H,
                                       kcache.shape[2], d_pos.data_ptr(), ps, _stream()), "mg_attn_decode_bf16")
    return out


PREFIX_CHUNK, PREFIX_PART = 64, 264                                     # include/magma_hip.h MG_PREFIX_CHUNK, MG_PREFIX_PART


def prefix_chunks(n_prefix: int) -> int:
    """Chunks the shared-prefix kernels cut a prefix of ``n_prefix`` positions into: a function of n_prefix alone."""
    return -(-int(n_prefix) // PREFIX_CHUNK)


def prefix_part(B: int, H: int, n_prefix: int, device) -> torch.Tensor:
    """The partials buffer of attn_decode_prefix for B rows: fp32 [B, H, n_chunk, PREFIX_PART] = (o[256], m, l, unused)."""
    return torch.zeros(B, H, prefix_chunks(n_prefix), PREFIX_PART, dtype=torch.float32, device=device)


def _shared_part(shared, B, H):
    n_prefix, part = shared
    assert part.dtype == torch.float32 and part.is_contiguous()
    if part.numel() < B * H * prefix_chunks(max(int(n_prefix), 1)) * PREFIX_PART:
        raise ValueError(f"the partials buffer holds {part.numel()} floats, {B} rows x {H} heads behind {n_prefix} positions need more")
    return int(n_prefix), part


def attn_decode_prefix(qkv, kprefix, vprefix, part, B, H, n_prefix, d_pos, rot_dim, sin_t, cos_t, *, pos_stride: int = 1):
    """Shared session prefix, kernel 1 (mg_attn_decode_prefix_bf16): the partial attention (m, l, o per chunk of PREFIX_CHUNK keys)
    of all B <= 16 rows of the fused ``qkv`` over positions [0, n_prefix) of the ONE prefix ``kprefix`` / ``vprefix``
    [H, S_prefix, 256], into ``part`` (prefix_part).  Row b's q is rotated at max(d_pos[b], n_prefix)."""
    _need_gpu(qkv, kprefix, vprefix, part)
    ps = _pos_stride(d_pos, B, pos_stride)
    assert kprefix.dtype == BF16 and kprefix.is_contiguous() and kprefix.ndim == 3 and kprefix.shape[2] == 256
    assert vprefix.dtype == BF16 and vprefix.is_contiguous() and vprefix.shape == kprefix.shape and kprefix.shape[0] == H
    n_prefix, part = _shared_part((n_prefix, part), B, H)
    check(L.load().mg_attn_decode_prefix_bf16(qkv.data_ptr(), kprefix.data_ptr(), vprefix.data_ptr(), part.data_ptr(), B, H, n_prefix,
                                              kprefix.shape[1], d_pos.data_ptr(), rot_dim, sin_t.data_ptr(), cos_t.data_ptr(), ps,
                                              _stream()), "mg_attn_decode_prefix_bf16")
    return part


def attn_decode_fused(qkv, kcache, vcache, out, B, H, d_pos, rot_dim, sin_t, cos_t, *, pos_stride: int = 0, shared=None):
    """rotary(q,k) + KV append at pos_b + attention over [0, pos_b], one launch; pos_b = d_pos[b * pos_stride].
    ``shared`` = (n_prefix, part) (mg_attn_decode_fused_shared_bf16): the caches hold the rows' OWN positions -- the append goes to own
    index pos_b - n_prefix, the attention over the own keys is merged with the prefix partials ``part`` of attn_decode_prefix."""
    _need_gpu(qkv)
    ps = _pos_stride(d_pos, B, pos_stride)
    if shared is not None:
        n_prefix, part = _shared_part(shared, B, H)
        check(L.load().mg_attn_decode_fused_shared_bf16(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), B, H,
                                                        kcache.shape[2], d_pos.data_ptr(), rot_dim, sin_t.data_ptr(),
                                                        cos_t.data_ptr(), ps, n_prefix, part.data_ptr(), _stream()),
              "mg_attn_decode_fused_shared_bf16")
        return out
    check(L.load().mg_attn_decode_fused_bf16(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), B, H,
                                             kcache.shape[2], d_pos.data_ptr(), rot_dim, sin_t.data_ptr(),
                                             cos_t.data_ptr(), ps, _stream()), "mg_attn_decode_fused_bf16")
    return out


def attn_decode_chunk(qkv, kcache, vcache, out, B, T, H, d_pos, rot_dim, sin_t, cos_t, *, pos_stride: int = 0):
    """attn_decode_fused for T consecutive positions of every sequence in one launch (mg_attn_decode_chunk_bf16): ``qkv``
    (B * T, 3 * H * 256) sequence-major, row b * T + t at position pos_b + t; k, v appended at [pos_b, pos_b + T), query t attends
    over [0, pos_b + t].  ``out`` (B * T, H * 256) may be a column range of wider rows.  Same bits as T successive attn_decode_fused
    launches for finite K / V (a later row's v enters an earlier query's sum as 0.f * v, so an Inf or NaN there would reach it);
    a row whose position lies outside [0, Smax) is skipped alone."""
    _need_gpu(qkv)
    ps = _pos_stride(d_pos, B, pos_stride)
    assert out.ndim == 2 and out.stride(1) == 1 and out.shape[1] == H * 256
    check(L.load().mg_attn_decode_chunk_bf16(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), out.stride(0), B, T,
                                             H, kcache.shape[2], d_pos.data_ptr(), rot_dim, _p(sin_t), _p(cos_t), ps, _stream()),
          "mg_attn_decode_chunk_bf16")
    return out


def argmax(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _need_gpu(logits)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    if out is None:
        out = torch.empty(logits.shape[0], dtype=torch.int64, device=logits.device)
    check(L.load().mg_argmax_f32(logits.data_ptr(), logits.stride(0), logits.shape[0], logits.shape[1],
                                 out.data_ptr(), _stream()), "mg_argmax_f32")
    return out


def sample(logits: torch.Tensor, temperature: float, top_k: int, top_p: float, seed: Optional[torch.Tensor],
           state: Optional[torch.Tensor], out: Optional[torch.Tensor] = None, filtered: Optional[torch.Tensor] = None,
           want_token: bool = True):
    """reference sampling.py:99-107 on the device: top-k filter, the reference's top-p rule, softmax(logits / temperature)
    and one multinomial draw per row (Philox stream keyed by ``seed`` at counter (state[0], row)).  ``filtered`` receives
    the filtered logits (the tensor the reference's filters return) when given."""
    _need_gpu(logits, seed, state, out, filtered)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    B, V = logits.shape
    if want_token and out is None:
        out = torch.empty(B, dtype=torch.int64, device=logits.device)
    if filtered is not None:
        assert filtered.dtype == torch.float32 and filtered.shape == logits.shape and filtered.stride(1) == 1
    check(L.load().mg_sample_f32(logits.data_ptr(), logits.stride(0), B, V, float(temperature), int(top_k), float(top_p),
                                 _p(seed), _p(state), _p(out) if want_token else None, _p(filtered),
                                 0 if filtered is None else filtered.stride(0), _stream()), "mg_sample_f32")
    return out


def sample_warp(logits: torch.Tensor, temperature: float, top_k: int, top_p: float, min_p: float, seed: Optional[torch.Tensor],
                state: Optional[torch.Tensor], out: Optional[torch.Tensor] = None, filtered: Optional[torch.Tensor] = None,
                want_token: bool = True):
    """transformers' sampler on the device (DESIGN.md "transformers' sampler"): temperature, top-k with every tie kept, nucleus
    top-p, min-p (sampling.py top_k_filter_ties / nucleus_filter / min_p_filter), softmax and one multinomial draw per row on the
    stream of ``sample``.  ``filtered`` receives the logits with -inf where a rule dropped the token."""
    _need_gpu(logits, seed, state, out, filtered)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    B, V = logits.shape
    if want_token and out is None:
        out = torch.empty(B, dtype=torch.int64, device=logits.device)
    if filtered is not None:
        assert filtered.dtype == torch.float32 and filtered.shape == logits.shape and filtered.stride(1) == 1
    check(L.load().mg_sample_warp_f32(logits.data_ptr(), logits.stride(0), B, V, float(temperature), int(top_k), float(top_p),
                                      float(min_p), _p(seed), _p(state), _p(out) if want_token else None, _p(filtered),
                                      0 if filtered is None else filtered.stride(0), _stream()), "mg_sample_warp_f32")
    return out


SAMPLE_ROW_BYTES = 32                                                   # include/magma_hip.h MG_SAMPLE_ROW_BYTES


def sample_rows_table(temperature, top_k, top_p, min_p, seed) -> torch.Tensor:
    """The host image of mg_sample_rows_f32's table, uint8 [R, SAMPLE_ROW_BYTES], from five sequences of R values: per row
    {double top_p, double log(min_p) (-inf: off), uint64 seed, float temperature, int32 top_k}.  The logarithm is math.log -- the C
    library's, which mg_sample_warp_f32 calls on its ``min_p`` -- so a row's min-p bound has the flat call's bits."""
    import math
    import struct
    rows = list(zip(temperature, top_k, top_p, min_p, seed))
    raw = b"".join(struct.pack("<ddQfi", float(p), math.log(float(m)) if float(m) > 0.0 else -math.inf,
                               int(s) & 0xffffffffffffffff, float(t), int(k)) for t, k, p, m, s in rows)
    assert len(raw) == SAMPLE_ROW_BYTES * len(rows)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(len(rows), SAMPLE_ROW_BYTES)


def sample_rows(logits: torch.Tensor, params: torch.Tensor, state: torch.Tensor, warp: bool = False,
                out: Optional[torch.Tensor] = None, filtered: Optional[torch.Tensor] = None, want_token: bool = True,
                slot: Optional[torch.Tensor] = None, finish: Optional[torch.Tensor] = None, history_cols: int = 0):
    """``sample`` (``warp``: ``sample_warp``) with every row's temperature, top_k, top_p, min_p and seed read from the device
    table ``params`` (sample_rows_table; mg_sample_rows_f32; DESIGN.md "Per-request sampling"): row r draws at the Philox counter
    (j, 0) under its own seed -- j = ``state[0]``, or with ``slot`` / ``finish`` (a slot session's tables, ``history_cols`` its
    ring) the occupant's own token index, idle rows skipped --, so it selects what the flat call on that row alone selects at
    step j.  A row with temperature 0 takes its first maximum.  Enqueue-only."""
    _need_gpu(logits, params, state, out, filtered, slot, finish)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    R, V = logits.shape
    assert params.dtype == torch.uint8 and params.is_contiguous() and params.shape == (R, SAMPLE_ROW_BYTES)
    assert state.dtype == torch.int32 and state.numel() >= 1
    if want_token and out is None:
        out = torch.empty(R, dtype=torch.int64, device=logits.device)
    if want_token:
        assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() == R
    if filtered is not None:
        assert filtered.dtype == torch.float32 and filtered.shape == logits.shape and filtered.stride(1) == 1
    for t in (slot, finish):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.shape == (R, 2))
    check(L.load().mg_sample_rows_f32(logits.data_ptr(), logits.stride(0), R, V, int(bool(warp)), params.data_ptr(), _p(state),
                                      _p(slot), _p(finish), int(history_cols), _p(out) if want_token else None, _p(filtered),
                                      0 if filtered is None else filtered.stride(0), _stream()), "mg_sample_rows_f32")
    return out


def sample_chunk(logits: torch.Tensor, T: int, params: torch.Tensor, count: torch.Tensor, finish: torch.Tensor,
                 n_draft: Optional[torch.Tensor] = None, history_cols: int = 0, warp: bool = False,
                 out: Optional[torch.Tensor] = None, filtered: Optional[torch.Tensor] = None, want_token: bool = True):
    """The selection launch of a speculative step (mg_sample_chunk_f32; DESIGN.md "Speculative decoding"): ``logits`` [B * T, V]
    holds T fed rows per sequence, ``params`` (sample_rows_table) ONE record per sequence.  Fed row b * T + t is selected under
    record b at the Philox counter (``count[b]`` + t, 0) -- what ``sample_rows`` selects on that row alone at ``state[0] =
    count[b] + t``.  Rows of a finished sequence (``finish[b, 0] >= 0``), of a sequence whose count lies outside
    ``[0, history_cols]`` and rows t > ``n_draft[b]`` (None: 0) are skipped whole: no logit read, ``out`` and ``filtered`` left
    alone.  ``T=1`` with a zero count is the arming call's selection.  Enqueue-only."""
    _need_gpu(logits, params, count, finish, n_draft, out, filtered)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    R, V = logits.shape
    T = int(T)
    assert T >= 1 and R % T == 0
    B = R // T
    assert params.dtype == torch.uint8 and params.is_contiguous() and params.shape == (B, SAMPLE_ROW_BYTES)
    for t, n in ((count, B), (finish, 2 * B), (n_draft, B)):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n)
    if want_token and out is None:
        out = torch.empty(R, dtype=torch.int64, device=logits.device)
    if want_token:
        assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= R
    if filtered is not None:
        assert filtered.dtype == torch.float32 and filtered.shape == logits.shape and filtered.stride(1) == 1
    check(L.load().mg_sample_chunk_f32(logits.data_ptr(), logits.stride(0), B, T, V, int(bool(warp)), params.data_ptr(), _p(count),
                                       _p(n_draft), _p(finish), int(history_cols), _p(out) if want_token else None, _p(filtered),
                                       0 if filtered is None else filtered.stride(0), _stream()), "mg_sample_chunk_f32")
    return out


def sample_finish(token: torch.Tensor, eos: int, state: torch.Tensor, d_pos: Optional[torch.Tensor] = None, delta: int = 1,
                  history: Optional[torch.Tensor] = None, clear: Optional[torch.Tensor] = None, clear_stride: int = 1, *,
                  pos_stride: int = 0):
    """Bookkeeping of one token step: first all-eos step, step counter, (optionally) KV write position += delta and the
    token history [B, n_steps] int64.  ``pos_stride=1``: d_pos holds one position per row and every one advances."""
    _need_gpu(token, state, d_pos, history)
    ps = 0 if d_pos is None else _pos_stride(d_pos, token.numel(), pos_stride)
    assert token.dtype == torch.int64 and state.dtype == torch.int32 and state.numel() >= 2
    if history is not None:
        assert history.dtype == torch.int64 and history.ndim == 2 and history.stride(1) == 1 and history.shape[0] == token.numel()
    if clear is not None:
        assert clear.dtype == torch.int32 and clear.is_contiguous()
    check(L.load().mg_sample_finish(token.data_ptr(), token.numel(), int(eos), state.data_ptr(), _p(d_pos), delta, _p(history),
                                    0 if history is None else history.stride(0), 0 if history is None else history.shape[1],
                                    _p(clear), 0 if clear is None else clear.numel() // clear_stride, clear_stride, ps, _stream()),
          "mg_sample_finish")


STOP_MAX_EOS, STOP_MAX_SEQ, STOP_MAX_LEN = 8, 16, 16                   # include/magma_hip.h MG_STOP_*
STOP_TABLE_INTS = STOP_MAX_EOS + STOP_MAX_SEQ + STOP_MAX_SEQ * STOP_MAX_LEN
STOP_EOS, STOP_SEQ = 0x100, 0x200                                       # finish[b][1] = reason | index


def stop_table(eos_ids, stop_seqs=()) -> torch.Tensor:
    """The host image of mg_sample_finish_rows' table (int32 [STOP_TABLE_INTS]): eos ids | sequence lengths | sequence tokens."""
    eos_ids, stop_seqs = [int(t) for t in eos_ids], [[int(t) for t in q] for q in stop_seqs]
    assert 1 <= len(eos_ids) <= STOP_MAX_EOS and len(stop_seqs) <= STOP_MAX_SEQ
    assert all(1 <= len(q) <= STOP_MAX_LEN for q in stop_seqs)
    t = torch.zeros(STOP_TABLE_INTS, dtype=torch.int32)
    t[: len(eos_ids)] = torch.tensor(eos_ids, dtype=torch.int32)
    for j, q in enumerate(stop_seqs):
        t[STOP_MAX_EOS + j] = len(q)
        off = STOP_MAX_EOS + STOP_MAX_SEQ + j * STOP_MAX_LEN
        t[off: off + len(q)] = torch.tensor(q, dtype=torch.int32)
    return t


def sample_finish_rows(token: torch.Tensor, state: torch.Tensor, table: torch.Tensor, n_eos: int, n_seq: int, pad: int,
                       finish: torch.Tensor, d_pos: Optional[torch.Tensor] = None, delta: int = 1,
                       history: Optional[torch.Tensor] = None, clear: Optional[torch.Tensor] = None, clear_stride: int = 1, *,
                       pos_stride: int = 0):
    """sample_finish with per-row stopping (mg_sample_finish_rows; host statement: sampling.stop_update): a row whose
    ``finish[b, 0]`` >= 0 gets ``pad`` into ``token[b]`` (in place) and its history; any other row's token is recorded and tested
    against the first ``n_eos`` eos ids and ``n_seq`` stop sequences of the device ``table`` (stop_table), and
    ``finish[b] = (step, STOP_EOS | i or STOP_SEQ | j)`` when it finishes.  ``state[1]`` records the first step at which no row
    is unfinished.  Enqueue-only."""
    _need_gpu(token, state, table, finish, d_pos, history)
    B = token.numel()
    ps = 0 if d_pos is None else _pos_stride(d_pos, B, pos_stride)
    assert token.dtype == torch.int64 and token.is_contiguous() and state.dtype == torch.int32 and state.numel() >= 2
    assert table.dtype == torch.int32 and table.is_contiguous() and table.numel() >= STOP_TABLE_INTS
    assert finish.dtype == torch.int32 and finish.is_contiguous() and finish.shape == (B, 2)
    if history is not None:
        assert history.dtype == torch.int64 and history.ndim == 2 and history.stride(1) == 1 and history.shape[0] == B
    if clear is not None:
        assert clear.dtype == torch.int32 and clear.is_contiguous()
    check(L.load().mg_sample_finish_rows(token.data_ptr(), B, state.data_ptr(), _p(d_pos), delta, _p(history),
                                         0 if history is None else history.stride(0), 0 if history is None else history.shape[1],
                                         _p(clear), 0 if clear is None else clear.numel() // clear_stride, clear_stride, ps,
                                         table.data_ptr(), int(n_eos), int(n_seq), int(pad), finish.data_ptr(), _stream()),
          "mg_sample_finish_rows")


def spec_finish(ids: torch.Tensor, n_draft: torch.Tensor, token: torch.Tensor, history: torch.Tensor, count: torch.Tensor,
                finish: torch.Tensor, table: torch.Tensor, n_eos: int, limit: int, lookup: torch.Tensor, lookup_len: torch.Tensor,
                stats: torch.Tensor, state: torch.Tensor, num_tokens: int, max_ngram: int, vocab: int,
                d_pos: Optional[torch.Tensor] = None, *, arm: bool = False, n_seq: Optional[int] = None):
    """The bookkeeping launch of a speculative step (mg_spec_finish; host statement: sampling.speculate_update): accepts the
    longest prefix of the drafts ``ids[b, 1:1 + n_draft[b]]`` that the step's argmaxes ``token`` (B * T) agree with, records the
    emitted tokens in ``history`` / ``count`` / ``finish`` / ``stats``, advances ``d_pos`` by their number and writes the next
    step's ``ids`` and ``n_draft`` by the prompt-lookup rule over ``lookup[b, :lookup_len[b]] ++ history[b, :count[b]]``.
    ``arm=True``: ``token`` holds the prefill's B selected tokens, nothing was fed (``d_pos`` is left alone).  ``n_seq`` (not
    None: mg_spec_finish_seq): every emitted token is also tested against the first ``n_seq`` stop sequences of ``table``, as
    sample_finish_rows tests a step's token.  Enqueue-only."""
    _need_gpu(ids, n_draft, token, history, count, finish, table, lookup, lookup_len, stats, state, d_pos)
    B, T = ids.shape
    assert ids.dtype == torch.int64 and ids.is_contiguous() and token.dtype == torch.int64 and token.is_contiguous()
    assert token.numel() >= (B if arm else B * T)
    assert history.dtype == torch.int64 and history.ndim == 2 and history.stride(1) == 1 and history.shape[0] == B
    assert lookup.dtype == torch.int32 and lookup.ndim == 2 and lookup.shape[0] == B and (lookup.shape[1] == 0 or lookup.stride(1) == 1)
    for t, n in ((n_draft, B), (count, B), (lookup_len, B), (finish, 2 * B), (stats, 3 * B)):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n
    assert state.dtype == torch.int32 and state.numel() >= 2
    assert table.dtype == torch.int32 and table.is_contiguous() and table.numel() >= STOP_TABLE_INTS
    if d_pos is not None:
        _pos_stride(d_pos, B, 1)
    head = (ids.data_ptr(), B, T, n_draft.data_ptr(), token.data_ptr(), 1 if arm else T, history.data_ptr(), history.stride(0),
            history.shape[1], count.data_ptr(), finish.data_ptr(), table.data_ptr(), int(n_eos))
    tail = (int(limit), None if arm else _p(d_pos), lookup.data_ptr() if lookup.shape[1] else None,
            lookup.stride(0) if lookup.shape[1] else 0, lookup.shape[1], lookup_len.data_ptr(), stats.data_ptr(), state.data_ptr(),
            int(num_tokens), int(max_ngram), int(vocab), _stream())
    if n_seq is None:
        check(L.load().mg_spec_finish(*head, *tail), "mg_spec_finish")
    else:
        check(L.load().mg_spec_finish_seq(*head, int(n_seq), *tail), "mg_spec_finish_seq")


STOP_LEN = 0x300                                                        # include/magma_hip.h MG_STOP_LEN: the budget ran out
SLOTS_MAX = 16                                                          # include/magma_hip.h MG_SLOTS_MAX


def sample_finish_slots(token: torch.Tensor, state: torch.Tensor, table: torch.Tensor, n_eos: int, n_seq: int, pad: int,
                        finish: torch.Tensor, slot: torch.Tensor, history: torch.Tensor, d_pos: Optional[torch.Tensor] = None,
                        delta: int = 1):
    """The bookkeeping launch of a slot session (mg_sample_finish_slots; host statement: sampling.slot_update):
    sample_finish_rows with a per-row window ``slot`` int32 [B, 2] = (begin column, token budget), ``history`` read and written as
    a ring of ``history.shape[1]`` columns, and positions that advance only for rows still open after this step.  A row whose
    own tokens reach its budget without a match finishes with ``STOP_LEN``.  Enqueue-only."""
    _need_gpu(token, state, table, finish, slot, d_pos, history)
    B = token.numel()
    assert token.dtype == torch.int64 and token.is_contiguous() and state.dtype == torch.int32 and state.numel() >= 2
    assert table.dtype == torch.int32 and table.is_contiguous() and table.numel() >= STOP_TABLE_INTS
    assert finish.dtype == torch.int32 and finish.is_contiguous() and finish.shape == (B, 2)
    assert slot.dtype == torch.int32 and slot.is_contiguous() and slot.shape == (B, 2)
    assert history.dtype == torch.int64 and history.ndim == 2 and history.stride(1) == 1 and history.shape[0] == B
    if d_pos is not None:
        _pos_stride(d_pos, B, 1)
    check(L.load().mg_sample_finish_slots(token.data_ptr(), B, state.data_ptr(), _p(d_pos), delta, history.data_ptr(),
                                          history.stride(0), history.shape[1], None, 0, 1, 1, table.data_ptr(), int(n_eos),
                                          int(n_seq), int(pad), finish.data_ptr(), slot.data_ptr(), _stream()),
          "mg_sample_finish_slots")


def slots_admit(kstage: torch.Tensor, vstage: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, src_row, dst_slot, lens,
                first_token: torch.Tensor, limits, state: torch.Tensor, d_pos: torch.Tensor, token: torch.Tensor,
                finish: torch.Tensor, slot: torch.Tensor, history: torch.Tensor, table: torch.Tensor, n_eos: int, n_seq: int,
                pos0: int = 0, dst0: Optional[int] = None):
    """Install n staged requests into slots of a slot session in one launch (mg_slots_admit_bf16): K / V positions [0, lens[j])
    of staging row ``src_row[j]`` ([L, n_stage, H, S_stage, 256]) go to live row ``dst_slot[j]`` ([L, B, H, Smax, 256]); the slot's
    position, token (``first_token[j]``, on the device), window, history column and finish record are set as the header states.
    ``src_row``, ``dst_slot``, ``lens`` and ``limits`` are host integers; what they must satisfy is checked by the entry point.
    ``pos0`` > 0 (a session prefix; mg_slots_admit_at_bf16): positions [pos0, pos0 + lens[j]) move instead, to the same positions
    of the slot, whose position becomes pos0 + lens[j]; nothing below pos0 is read or written.
    ``dst0`` (a live cache that holds the rows' own positions only; mg_slots_admit_shared_bf16): staged positions
    [pos0, pos0 + lens[j]) go to live positions [dst0, dst0 + lens[j]) instead; the slot's position is still pos0 + lens[j]."""
    _need_gpu(kstage, vstage, kcache, vcache, first_token, state, d_pos, token, finish, slot, history, table)
    Lr, n_stage, H, S_stage, hd = kstage.shape
    _, B, _, Smax, _ = kcache.shape
    assert hd == 256 and kcache.shape[4] == 256 and (kcache.shape[0], kcache.shape[2]) == (Lr, H)
    assert vstage.shape == kstage.shape and vcache.shape == kcache.shape
    assert all(t.dtype == BF16 and t.is_contiguous() for t in (kstage, vstage, kcache, vcache))
    n = len(src_row)
    assert len(dst_slot) == len(lens) == len(limits) == n
    assert first_token.dtype == torch.int64 and first_token.is_contiguous()
    if first_token.numel() < n:
        raise ValueError(f"first_token holds {first_token.numel()} tokens for {n} requests")
    assert state.dtype == torch.int32 and state.numel() >= 2 and token.dtype == torch.int64 and token.is_contiguous()
    assert d_pos.dtype == torch.int32 and d_pos.is_contiguous() and d_pos.numel() >= B and token.numel() >= B
    assert finish.dtype == torch.int32 and finish.is_contiguous() and finish.shape == (B, 2)
    assert slot.dtype == torch.int32 and slot.is_contiguous() and slot.shape == (B, 2)
    assert history.dtype == torch.int64 and history.ndim == 2 and history.stride(1) == 1 and history.shape[0] == B
    assert table.dtype == torch.int32 and table.is_contiguous() and table.numel() >= STOP_TABLE_INTS
    arr = lambda xs: (C.c_int32 * max(n, 1))(*[int(x) for x in xs])  # noqa: E731
    args = (kstage.data_ptr(), vstage.data_ptr(), n_stage, S_stage, kcache.data_ptr(), vcache.data_ptr(), Lr, B, H, Smax, n,
            arr(src_row), arr(dst_slot), arr(lens), first_token.data_ptr(), arr(limits), state.data_ptr(), d_pos.data_ptr(),
            token.data_ptr(), finish.data_ptr(), slot.data_ptr(), history.data_ptr(), history.stride(0), history.shape[1],
            table.data_ptr(), int(n_eos), int(n_seq))
    if dst0 is not None:
        check(L.load().mg_slots_admit_shared_bf16(*args, int(pos0), int(dst0), _stream()), "mg_slots_admit_shared_bf16")
    elif pos0:
        check(L.load().mg_slots_admit_at_bf16(*args, int(pos0), _stream()), "mg_slots_admit_at_bf16")
    else:
        check(L.load().mg_slots_admit_bf16(*args, _stream()), "mg_slots_admit_bf16")


def advance_pos(d_pos: torch.Tensor, delta: int = 1, *, pos_stride: int = 0):
    """d_pos[0] += delta; with ``pos_stride=1`` every entry of d_pos (one position per row) += delta."""
    ps = _pos_stride(d_pos, d_pos.numel(), pos_stride)
    check(L.load().mg_advance_pos(d_pos.data_ptr(), delta, d_pos.numel(), ps, _stream()), "mg_advance_pos")


def logits_process(logits: torch.Tensor, state: torch.Tensor, history: Optional[torch.Tensor], *, repetition_penalty: float = 1.0,
                   no_repeat_ngram_size: int = 0, min_new_tokens: int = 0, eos: int = -1,
                   suppress: Optional[torch.Tensor] = None, n_suppress: Optional[int] = None, normalize: bool = False,
                   eos_more: Optional[torch.Tensor] = None, n_eos_more: Optional[int] = None):
    """The logits processors (mg_logits_process_f32; host statement: sampling.process_logits) in place on the fp32 rows
    ``logits`` (R, V): repetition penalty, no-repeat n-gram, min-new-tokens, suppress, in transformers' order.  ``state[0]`` is
    the step (tokens generated so far, read on the device), ``history`` (R, >= step) int64 the rows' tokens, ``suppress`` a
    device int32 array of which the first ``n_suppress`` (default: all) ids count.  ``normalize``: log_softmax first (the beam
    form, for beam_topk(normalized=True)).  ``eos_more``: a device int32 array of which the first ``n_eos_more`` (default: all,
    at most 8) are further eos ids the min-new-tokens rule bans (None: ``eos`` alone).  Enqueue-only."""
    _need_gpu(logits, state, history, suppress, eos_more)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    assert state.dtype == torch.int32 and state.numel() >= 1
    R, V = logits.shape
    if history is not None:
        assert history.dtype == torch.int64 and history.ndim == 2 and history.stride(1) == 1 and history.shape[0] == R
    if suppress is not None:
        assert suppress.dtype == torch.int32 and suppress.is_contiguous()
    ns = (0 if suppress is None else suppress.numel()) if n_suppress is None else int(n_suppress)
    assert ns == 0 or (suppress is not None and ns <= suppress.numel())
    if eos_more is not None:
        assert eos_more.dtype == torch.int32 and eos_more.is_contiguous()
    nm = (0 if eos_more is None else eos_more.numel()) if n_eos_more is None else int(n_eos_more)
    assert nm == 0 or (eos_more is not None and nm <= eos_more.numel())
    check(L.load().mg_logits_process_f32(logits.data_ptr(), logits.stride(0), R, V, state.data_ptr(), _p(history),
                                         0 if history is None else history.stride(0), 0 if history is None else history.shape[1],
                                         float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens), int(eos),
                                         _p(suppress), ns, 1 if normalize else 0, _p(eos_more) if nm else None, nm, _stream()),
          "mg_logits_process_f32")
    return logits


TRIE_MAX_LEN = 64           # include/magma_hip.h MG_TRIE_MAX_LEN: the longest sequence of a token trie, columns of the path cache


def trie_path(R: int, device) -> torch.Tensor:
    """The per-row path cache of logits_process_constrained (int32 [R, TRIE_MAX_LEN]; any contents do)."""
    return torch.zeros(R, TRIE_MAX_LEN, dtype=torch.int32, device=device)


def logits_process_constrained(logits: torch.Tensor, state: torch.Tensor, history: torch.Tensor, table: torch.Tensor,
                               roots: torch.Tensor, path: torch.Tensor, *, repetition_penalty: float = 1.0,
                               no_repeat_ngram_size: int = 0, min_new_tokens: int = 0, eos: int = -1,
                               suppress: Optional[torch.Tensor] = None, n_suppress: Optional[int] = None,
                               eos_more: Optional[torch.Tensor] = None, n_eos_more: Optional[int] = None):
    """logits_process (its rules, its arguments; no beam form) followed in the same launch by the trie constraint
    (mg_logits_process_constrained_f32; host statement: sampling.constrain_logits): row r keeps the tokens that continue the walk
    of ``history[r, :state[0]]`` from node ``roots[r]`` (device int32 [R]) through ``table`` (device int32: sampling.TokenTrie.flat()
    / trie_forest(), read at run time) and -- at a terminal node or off the trie -- ``eos`` and the ``eos_more`` ids; every other
    column becomes -inf.  ``path`` (trie_path): the launch's per-row cache, checked before use -- any contents give the same
    result.  Enqueue-only."""
    _need_gpu(logits, state, history, suppress, eos_more, table, roots, path)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    assert state.dtype == torch.int32 and state.numel() >= 1
    R, V = logits.shape
    assert history.dtype == torch.int64 and history.ndim == 2 and history.stride(1) == 1 and history.shape[0] == R
    assert table.dtype == torch.int32 and table.is_contiguous() and table.ndim == 1 and table.numel() >= 2
    assert roots.dtype == torch.int32 and roots.is_contiguous() and roots.numel() >= R
    assert path.dtype == torch.int32 and path.is_contiguous() and path.ndim == 2 and path.shape[0] >= R and path.shape[1] == TRIE_MAX_LEN
    if suppress is not None:
        assert suppress.dtype == torch.int32 and suppress.is_contiguous()
    ns = (0 if suppress is None else suppress.numel()) if n_suppress is None else int(n_suppress)
    assert ns == 0 or (suppress is not None and ns <= suppress.numel())
    if eos_more is not None:
        assert eos_more.dtype == torch.int32 and eos_more.is_contiguous()
    nm = (0 if eos_more is None else eos_more.numel()) if n_eos_more is None else int(n_eos_more)
    assert nm == 0 or (eos_more is not None and nm <= eos_more.numel())
    check(L.load().mg_logits_process_constrained_f32(logits.data_ptr(), logits.stride(0), R, V, state.data_ptr(), history.data_ptr(),
                                                     history.stride(0), history.shape[1], float(repetition_penalty),
                                                     int(no_repeat_ngram_size), int(min_new_tokens), int(eos), _p(suppress), ns,
                                                     _p(eos_more) if nm else None, nm, table.data_ptr(), table.numel(),
                                                     roots.data_ptr(), path.data_ptr(), _stream()),
          "mg_logits_process_constrained_f32")
    return logits


def _slot_operands(R: int, state: torch.Tensor, history: torch.Tensor, slot: torch.Tensor, finish: torch.Tensor):
    """The checks the three slot launches share: the state, the ring history and the tables sample_finish_slots keeps."""
    assert state is not None and state.dtype == torch.int32 and state.numel() >= 1
    assert history.dtype == torch.int64 and history.ndim == 2 and history.stride(1) == 1 and history.shape[0] == R
    assert slot.dtype == torch.int32 and slot.is_contiguous() and slot.shape == (R, 2)
    assert finish.dtype == torch.int32 and finish.is_contiguous() and finish.shape == (R, 2)


def _counted(t: Optional[torch.Tensor], n: Optional[int]) -> int:
    """How many leading entries of the device int32 array ``t`` count (default: all)."""
    if t is not None:
        assert t.dtype == torch.int32 and t.is_contiguous()
    n = (0 if t is None else t.numel()) if n is None else int(n)
    assert n == 0 or (t is not None and n <= t.numel())
    return n


def logits_process_slots(logits: torch.Tensor, state: torch.Tensor, history: torch.Tensor, slot: torch.Tensor, finish: torch.Tensor, *,
                         repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0, eos: int = -1,
                         suppress: Optional[torch.Tensor] = None, n_suppress: Optional[int] = None, normalize: bool = False,
                         eos_more: Optional[torch.Tensor] = None, n_eos_more: Optional[int] = None):
    """logits_process for the rows of a slot session (mg_logits_process_slots_f32; host statement of the window:
    sampling.slot_tokens): ``history`` is the ring, ``slot`` int32 [R, 2] = (begin column, budget) and ``finish`` int32 [R, 2] the
    tables sample_finish_slots keeps.  An occupied row gets the rules over its occupant's n tokens in ring order, with n as the
    step; an idle row (finish[r, 0] >= 0) keeps its bits.  Enqueue-only."""
    _need_gpu(logits, state, history, suppress, eos_more, slot, finish)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    R, V = logits.shape
    _slot_operands(R, state, history, slot, finish)
    ns, nm = _counted(suppress, n_suppress), _counted(eos_more, n_eos_more)
    check(L.load().mg_logits_process_slots_f32(logits.data_ptr(), logits.stride(0), R, V, state.data_ptr(), history.data_ptr(),
                                               history.stride(0), history.shape[1], float(repetition_penalty),
                                               int(no_repeat_ngram_size), int(min_new_tokens), int(eos), _p(suppress), ns,
                                               1 if normalize else 0, _p(eos_more) if nm else None, nm, slot.data_ptr(),
                                               finish.data_ptr(), _stream()),
          "mg_logits_process_slots_f32")
    return logits


def logits_process_constrained_slots(logits: torch.Tensor, state: torch.Tensor, history: torch.Tensor, table: torch.Tensor,
                                     roots: torch.Tensor, path: torch.Tensor, slot: torch.Tensor, finish: torch.Tensor, *,
                                     repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0,
                                     eos: int = -1, suppress: Optional[torch.Tensor] = None, n_suppress: Optional[int] = None,
                                     eos_more: Optional[torch.Tensor] = None, n_eos_more: Optional[int] = None):
    """logits_process_constrained for the rows of a slot session (mg_logits_process_constrained_slots_f32): the rules and the trie
    walk run over the occupant's window of the ring ``history`` (logits_process_slots); ``path`` rows of an earlier occupant fail
    their proof and are re-walked from ``roots[r]``.  An idle row keeps its bits.  Enqueue-only."""
    _need_gpu(logits, state, history, suppress, eos_more, table, roots, path, slot, finish)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    R, V = logits.shape
    _slot_operands(R, state, history, slot, finish)
    assert table.dtype == torch.int32 and table.is_contiguous() and table.ndim == 1 and table.numel() >= 2
    assert roots.dtype == torch.int32 and roots.is_contiguous() and roots.numel() >= R
    assert path.dtype == torch.int32 and path.is_contiguous() and path.ndim == 2 and path.shape[0] >= R and path.shape[1] == TRIE_MAX_LEN
    ns, nm = _counted(suppress, n_suppress), _counted(eos_more, n_eos_more)
    check(L.load().mg_logits_process_constrained_slots_f32(logits.data_ptr(), logits.stride(0), R, V, state.data_ptr(),
                                                           history.data_ptr(), history.stride(0), history.shape[1],
                                                           float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens),
                                                           int(eos), _p(suppress), ns, _p(eos_more) if nm else None, nm,
                                                           table.data_ptr(), table.numel(), roots.data_ptr(), path.data_ptr(),
                                                           slot.data_ptr(), finish.data_ptr(), _stream()),
          "mg_logits_process_constrained_slots_f32")
    return logits


def logits_guidance(cond: torch.Tensor, uncond: torch.Tensor, scale: float, min_p: float = 0.0):
    """Classifier-free guidance in place on the fp32 rows ``cond`` (R, V) against ``uncond`` (R, V), one launch of one workgroup
    per pair (mg_logits_guidance_f32; host statement: sampling.guide_logits): with c / u the log_softmax of the two rows,
    cond = u + scale * (c - u); a conditional -inf stays -inf; ``min_p`` > 0 also writes -inf where cond - max(cond) <
    log(min_p) (fp32 comparison against the fp32 rounding of the float64 log, on the raw conditional logits).  ``uncond`` is
    only read and must be finite; both are views of any row stride.  Enqueue-only."""
    _need_gpu(cond, uncond)
    assert cond.dtype == torch.float32 and cond.ndim == 2 and cond.stride(1) == 1
    assert uncond.dtype == torch.float32 and uncond.shape == cond.shape and uncond.stride(1) == 1
    R, V = cond.shape
    if not 0.0 <= float(min_p) <= 1.0:
        raise ValueError(f"min_p must lie in [0, 1], got {min_p!r}")
    log_min_p = float(torch.tensor(float(min_p), dtype=torch.float64).log().to(torch.float32)) if float(min_p) > 0.0 else float("-inf")
    check(L.load().mg_logits_guidance_f32(cond.data_ptr(), cond.stride(0) if R > 1 else max(cond.stride(0), V), uncond.data_ptr(),
                                          uncond.stride(0) if R > 1 else max(uncond.stride(0), V), R, V, float(scale), log_min_p,
                                          _stream()), "mg_logits_guidance_f32")
    return cond


def guidance_follow(token: torch.Tensor, d_pos: Optional[torch.Tensor], R: int, delta: int = 1, *, pos_stride: int = 1):
    """The negative half of a guided batch follows the guided half (mg_guidance_follow): token[R + r] = token[r] and, with
    ``d_pos`` and ``pos_stride=1``, d_pos[R + r] += delta, for r < R.  Runs after the bookkeeping launch.  Enqueue-only."""
    _need_gpu(token, d_pos)
    R = int(R)
    assert token.dtype == torch.int64 and token.is_contiguous() and R >= 1 and token.numel() >= 2 * R
    ps = 0 if d_pos is None else _pos_stride(d_pos, 2 * R, pos_stride)
    check(L.load().mg_guidance_follow(token.data_ptr(), _p(d_pos), R, int(delta), ps, _stream()), "mg_guidance_follow")
    return token


def beam_topk(logits: torch.Tensor, run: torch.Tensor, cand_score: torch.Tensor, cand_tok: torch.Tensor, normalized: bool = False):
    """Per row: the top K2 = cand_score.shape[1] scores run[row] + log_softmax(logits[row]) (score desc, lower token first).
    ``normalized``: the rows already hold log_softmax scores (logits_process(normalize=True)): candidates run[row] + logits[row]."""
    _need_gpu(logits, run, cand_score, cand_tok)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    R, V = logits.shape
    assert run.dtype == torch.float32 and run.is_contiguous() and run.numel() == R
    assert cand_score.dtype == torch.float32 and cand_tok.dtype == torch.int32 and cand_score.is_contiguous() and cand_tok.is_contiguous()
    assert cand_score.shape == cand_tok.shape and cand_score.ndim == 2 and cand_score.shape[0] == R
    name = "mg_beam_topk_scores_f32" if normalized else "mg_beam_topk_f32"
    check(getattr(L.load(), name)(logits.data_ptr(), logits.stride(0), R, V, run.data_ptr(), cand_score.shape[1],
                                  cand_score.data_ptr(), cand_tok.data_ptr(), _stream()), name)


LOGPROBS_MAX_TOP = 20                                                   # include/magma_hip.h MG_LOGPROBS_MAX_TOP


def token_logprobs(logits: torch.Tensor, token: torch.Tensor, lp: torch.Tensor, top_id: Optional[torch.Tensor] = None,
                   top_lp: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None):
    """Per row of the fp32 ``logits`` (R, V): log_softmax(logits[r])[token[r]] into column c of ``lp`` (R, cols) fp32 -- c =
    ``state[0]`` (device int32, read at run time) or 0 without a state -- and, when ``top_id`` (R, cols, n_top) int32 /
    ``top_lp`` (R, cols, n_top) fp32 are given, the row's n_top most probable tokens into [r, c, :], ranked by raw logit descending,
    lower id first (mg_token_logprobs_f32; host statement: sampling.token_logprobs).  c >= cols writes nothing; a token outside
    [0, V) gives -inf.  n_top must lie in [0, 20] and not exceed V.  Enqueue-only."""
    _need_gpu(logits, token, lp, top_id, top_lp, state)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    R, V = logits.shape
    assert token.dtype == torch.int64 and token.is_contiguous() and token.numel() == R
    assert lp.dtype == torch.float32 and lp.ndim == 2 and lp.shape[0] == R and lp.shape[1] >= 1
    assert lp.stride(1) == 1 and (R == 1 or lp.stride(0) >= lp.shape[1])
    cols = lp.shape[1]
    assert (top_id is None) == (top_lp is None), "top_id and top_lp come together"
    n_top = 0
    if top_id is not None:
        assert top_id.dtype == torch.int32 and top_lp.dtype == torch.float32 and top_id.is_contiguous() and top_lp.is_contiguous()
        assert top_id.ndim == 3 and top_id.shape[:2] == (R, cols) and top_lp.shape == top_id.shape
        n_top = top_id.shape[2]
    if state is not None:
        assert state.dtype == torch.int32 and state.numel() >= 1
    check(L.load().mg_token_logprobs_f32(logits.data_ptr(), logits.stride(0), R, V, token.data_ptr(), _p(state), lp.data_ptr(),
                                         lp.stride(0) if R > 1 else max(lp.stride(0), cols), cols, n_top,
                                         _p(top_id) if n_top else None, _p(top_lp) if n_top else None, _stream()),
          "mg_token_logprobs_f32")
    return lp


def token_logprobs_slots(logits: torch.Tensor, token: torch.Tensor, lp: torch.Tensor, top_id: Optional[torch.Tensor],
                         top_lp: Optional[torch.Tensor], state: torch.Tensor, slot: torch.Tensor, finish: torch.Tensor,
                         ring_cols: int):
    """token_logprobs for the rows of a slot session (mg_token_logprobs_slots_f32): an occupied row writes column n of ``lp`` /
    ``top_id`` / ``top_lp`` -- n = the tokens its occupant has generated before this step, from ``state[0]``, ``slot`` and
    ``finish`` (sample_finish_slots' tables) over a ring of ``ring_cols`` columns; column 0 belongs to the admission --, an idle
    row and a column >= lp.shape[1] write nothing.  Enqueue-only."""
    _need_gpu(logits, token, lp, top_id, top_lp, state, slot, finish)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    R, V = logits.shape
    assert token.dtype == torch.int64 and token.is_contiguous() and token.numel() == R
    assert lp.dtype == torch.float32 and lp.ndim == 2 and lp.shape[0] == R and lp.shape[1] >= 1
    assert lp.stride(1) == 1 and (R == 1 or lp.stride(0) >= lp.shape[1])
    cols = lp.shape[1]
    assert (top_id is None) == (top_lp is None), "top_id and top_lp come together"
    n_top = 0
    if top_id is not None:
        assert top_id.dtype == torch.int32 and top_lp.dtype == torch.float32 and top_id.is_contiguous() and top_lp.is_contiguous()
        assert top_id.ndim == 3 and top_id.shape[:2] == (R, cols) and top_lp.shape == top_id.shape
        n_top = top_id.shape[2]
    assert state is not None and state.dtype == torch.int32 and state.numel() >= 1
    assert slot.dtype == torch.int32 and slot.is_contiguous() and slot.shape == (R, 2)
    assert finish.dtype == torch.int32 and finish.is_contiguous() and finish.shape == (R, 2)
    check(L.load().mg_token_logprobs_slots_f32(logits.data_ptr(), logits.stride(0), R, V, token.data_ptr(), state.data_ptr(),
                                               lp.data_ptr(), lp.stride(0) if R > 1 else max(lp.stride(0), cols), cols, n_top,
                                               _p(top_id) if n_top else None, _p(top_lp) if n_top else None, slot.data_ptr(),
                                               finish.data_ptr(), int(ring_cols), _stream()),
          "mg_token_logprobs_slots_f32")
    return lp


def token_logprobs_rows(logits: torch.Tensor, row_of: torch.Tensor, token: torch.Tensor, lp: torch.Tensor):
    """token_logprobs with a row indirection (mg_token_logprobs_rows_f32): lp[i] = log_softmax(logits[row_of[i]])[token[i]] for N
    entries -- ``row_of`` / ``token`` int32 (N,), ``lp`` fp32 (N,) -- with the bits token_logprobs gives for that row and token; the
    edges out of one trie node share their parent's logits row.  A row outside the logits or a token outside [0, V) gives -inf."""
    _need_gpu(logits, row_of, token, lp)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    N = row_of.numel()
    assert row_of.dtype == torch.int32 and token.dtype == torch.int32 and row_of.is_contiguous() and token.is_contiguous()
    assert token.numel() == N and lp.dtype == torch.float32 and lp.is_contiguous() and lp.numel() == N
    check(L.load().mg_token_logprobs_rows_f32(logits.data_ptr(), logits.stride(0), logits.shape[0], logits.shape[1], row_of.data_ptr(),
                                              token.data_ptr(), N, lp.data_ptr(), _stream()), "mg_token_logprobs_rows_f32")
    return lp


EARLY_STOPPING_CODES = {False: 0, True: 1, "never": 2}


def _beam_state(cand_score, cand_tok, B, k, G, K2, state, bufs, d_pos, pos_stride):
    """The checked buffers of a beam bookkeeping launch as (mg_beam_state, pos_stride): beam_finish's (G = 1) and
    beam_finish_groups' share of the work."""
    R = B * k
    _need_gpu(cand_score, cand_tok, state, d_pos, *bufs.values())
    assert cand_score.shape == (R, K2) and cand_tok.shape == (R, K2)
    assert cand_score.dtype == torch.float32 and cand_tok.dtype == torch.int32 and cand_score.is_contiguous() and cand_tok.is_contiguous()
    ps = 0 if d_pos is None else _pos_stride(d_pos, R, pos_stride)
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    for name, dt, n in (("run", f32, R), ("fin_score", f32, R), ("fin_flag", i32, R), ("fin_len", i32, R), ("unsat", i32, B * G),
                        ("parent", i32, R), ("token", i64, R)):
        t = bufs[name]
        assert t.dtype == dt and t.is_contiguous() and t.numel() == n, name
    ld = bufs["hist"].shape[1]
    for name in ("fin_tok", "fin_stage", "hist", "hist_stage"):
        t = bufs[name]
        assert t.dtype == i64 and t.is_contiguous() and t.shape == (R, ld), name
    assert state.dtype == i32 and state.numel() >= 2
    bs = L.BeamState(*(bufs[n].data_ptr() for n in ("run", "fin_score", "fin_flag", "fin_len", "fin_tok", "fin_stage", "hist",
                                                    "hist_stage")), ld, bufs["unsat"].data_ptr(), bufs["parent"].data_ptr(),
                     bufs["token"].data_ptr())
    return bs, ps


def beam_finish(cand_score: torch.Tensor, cand_tok: torch.Tensor, B: int, k: int, V: int, eos: int, length_penalty: float,
                early_stopping, max_steps: int, state: torch.Tensor, bufs: dict, d_pos: Optional[torch.Tensor] = None,
                pos_stride: int = 0):
    """Beam bookkeeping of one token step (mg_beam_finish).  ``bufs``: run, fin_score, fin_flag, fin_len, fin_tok, fin_stage,
    hist, hist_stage, unsat, parent, token (BeamBuffers.as_dict())."""
    bs, ps = _beam_state(cand_score, cand_tok, B, k, 1, 2 * k, state, bufs, d_pos, pos_stride)
    es = EARLY_STOPPING_CODES[early_stopping]
    check(L.load().mg_beam_finish(cand_score.data_ptr(), cand_tok.data_ptr(), B, k, V, int(eos), float(length_penalty), es,
                                  int(max_steps), state.data_ptr(), _p(d_pos), ps, C.byref(bs), _stream()), "mg_beam_finish")


def beam_finish_groups(cand_score: torch.Tensor, cand_tok: torch.Tensor, B: int, k: int, G: int, diversity_penalty: float, V: int,
                       eos: int, length_penalty: float, early_stopping, max_steps: int, state: torch.Tensor, bufs: dict,
                       d_pos: Optional[torch.Tensor] = None, pos_stride: int = 0):
    """Bookkeeping of one token step of diverse beam search (mg_beam_finish_groups): beam_finish over k beams in ``G`` groups
    of k / G, group g's candidates less ``diversity_penalty`` times the number of earlier groups' beams that selected their token
    at this step.  The candidate lists hold K2 = cand_score.shape[1] entries per row: k + k / G (2k at G = 1, where the call
    writes what beam_finish writes); ``bufs`` as for beam_finish, with B * G entries in ``unsat``."""
    if G < 1 or k % G:
        raise ValueError(f"num_beam_groups = {G} must divide num_beams = {k}")
    bs, ps = _beam_state(cand_score, cand_tok, B, k, G, cand_score.shape[1], state, bufs, d_pos, pos_stride)
    es = EARLY_STOPPING_CODES[early_stopping]
    check(L.load().mg_beam_finish_groups(cand_score.data_ptr(), cand_tok.data_ptr(), B, k, G, cand_score.shape[1],
                                         float(diversity_penalty), V, int(eos), float(length_penalty), es, int(max_steps),
                                         state.data_ptr(), _p(d_pos), ps, C.byref(bs), _stream()), "mg_beam_finish_groups")


def kv_reorder(kcache: torch.Tensor, vcache: torch.Tensor, kstage: torch.Tensor, vstage: torch.Tensor, parent: torch.Tensor,
               d_pos: torch.Tensor, *, pos_stride: int = 0):
    """Row b of every layer's K / V cache [L, R, H, Smax, 256] gets positions [0, d_pos_b) of row parent[b] (parent[b] != b)."""
    _need_gpu(kcache, vcache, kstage, vstage, parent, d_pos)
    Lr, R, H, Smax, hd = kcache.shape
    assert hd == 256 and kcache.dtype == BF16 and all(t.shape == kcache.shape and t.dtype == BF16 and t.is_contiguous()
                                                      for t in (kcache, vcache, kstage, vstage))
    assert parent.dtype == torch.int32 and parent.is_contiguous() and parent.numel() == R
    ps = _pos_stride(d_pos, R, pos_stride)
    check(L.load().mg_kv_reorder_bf16(kcache.data_ptr(), vcache.data_ptr(), kstage.data_ptr(), vstage.data_ptr(), Lr, R, H, Smax,
                                      parent.data_ptr(), d_pos.data_ptr(), ps, _stream()), "mg_kv_reorder_bf16")


CONTRASTIVE_CHUNK, CONTRASTIVE_MAX_K = 32, 16                           # include/magma_hip.h MG_CONTRASTIVE_*


def contrastive_chunks(Tmax: int) -> int:
    """Context chunks per sample of a store of ``Tmax`` positions: the middle extent of contrastive_sim's ``part``."""
    return (Tmax + CONTRASTIVE_CHUNK - 1) // CONTRASTIVE_CHUNK


def contrastive_topk(logits: torch.Tensor, src: torch.Tensor, k: int, token: torch.Tensor, cand_p: torch.Tensor):
    """Per sample b the ``k`` most probable tokens of logits row ``src[b]`` (fp32 (B * k, V); ``src`` int32 (B,)), raw logit
    descending, lower id first, into ``token[b * k + j]`` (int64 (B * k,): the next step's input ids) and their fp32 softmax
    probabilities into ``cand_p`` (B, k) (mg_contrastive_topk_f32).  Enqueue-only."""
    _need_gpu(logits, src, token, cand_p)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    R, V = logits.shape
    B = src.numel()
    assert src.dtype == torch.int32 and src.is_contiguous()
    assert token.dtype == torch.int64 and token.is_contiguous() and token.numel() == B * k
    assert cand_p.dtype == torch.float32 and cand_p.is_contiguous() and cand_p.numel() == B * k
    check(L.load().mg_contrastive_topk_f32(logits.data_ptr(), logits.stride(0), R, V, src.data_ptr(), B, int(k), token.data_ptr(),
                                           cand_p.data_ptr(), _stream()), "mg_contrastive_topk_f32")


def _contrast_store(hidden, ctx, ctx_len, k):
    """The checked geometry (B, Tmax, d, n_chunk) of a contrastive launch's hidden rows and context store."""
    assert hidden.dtype == BF16 and hidden.ndim == 2 and hidden.stride(1) == 1
    assert ctx.dtype == BF16 and ctx.ndim == 3 and ctx.is_contiguous()
    B, Tmax, d = ctx.shape
    assert hidden.shape == (B * k, d), f"hidden must be ({B * k}, {d}), got {tuple(hidden.shape)}"
    assert ctx_len.dtype == torch.int32 and ctx_len.is_contiguous() and ctx_len.numel() == B
    return B, Tmax, d, contrastive_chunks(Tmax)


def contrastive_sim(hidden: torch.Tensor, ctx: torch.Tensor, ctx_len: torch.Tensor, k: int, part: torch.Tensor, len_max: int):
    """part[b, c, j] (fp32 (B, contrastive_chunks(Tmax), k)) = the largest cosine of candidate row ``hidden[b * k + j]`` (bf16
    (B * k, d)) with the valid positions (< ``ctx_len[b]``) of chunk c of ``ctx[b]`` (bf16 (B, Tmax, d)); -1e30 for a chunk without
    one (mg_contrastive_sim_bf16).  ``len_max``: the caller's host bound of ctx_len's entries (checked against Tmax; the device
    values are clamped).  Enqueue-only."""
    _need_gpu(hidden, ctx, ctx_len, part)
    B, Tmax, d, n_chunk = _contrast_store(hidden, ctx, ctx_len, k)
    assert part.dtype == torch.float32 and part.is_contiguous() and part.numel() == B * n_chunk * k
    check(L.load().mg_contrastive_sim_bf16(hidden.data_ptr(), hidden.stride(0), ctx.data_ptr(), B, Tmax, d, ctx_len.data_ptr(),
                                           int(len_max), int(k), part.data_ptr(), n_chunk, _stream()), "mg_contrastive_sim_bf16")
    return part


def contrastive_finish(part: torch.Tensor, cand_p: torch.Tensor, alpha: float, hidden: torch.Tensor, ctx: torch.Tensor,
                       ctx_len: torch.Tensor, src: torch.Tensor, token: torch.Tensor, eos: int, state: torch.Tensor, len_max: int,
                       d_pos: Optional[torch.Tensor] = None, delta: int = 1, history: Optional[torch.Tensor] = None, *,
                       pos_stride: int = 0):
    """The selection and the bookkeeping of a contrastive step (mg_contrastive_finish; host statement: sampling.contrastive_rank):
    per sample the first j with the largest (1 - alpha) * cand_p[b, j] - alpha * max_c part[b, c, j]; its token (``token[b * k + j]``)
    into column ``state[0]`` of the k history rows of the sample, ``src[b] = b * k + j``, its hidden row appended to ``ctx[b]``,
    ``ctx_len[b] += 1``; then sample_finish's bookkeeping over the B selected tokens, every row's position advanced."""
    _need_gpu(part, cand_p, hidden, ctx, ctx_len, src, token, state, d_pos, history)
    k = cand_p.shape[-1] if cand_p.ndim == 2 else 0
    B, Tmax, d, n_chunk = _contrast_store(hidden, ctx, ctx_len, k)
    assert cand_p.dtype == torch.float32 and cand_p.is_contiguous() and cand_p.shape == (B, k)
    assert part.dtype == torch.float32 and part.is_contiguous() and part.numel() == B * n_chunk * k
    assert src.dtype == torch.int32 and src.is_contiguous() and src.numel() == B
    assert token.dtype == torch.int64 and token.is_contiguous() and token.numel() == B * k
    assert state.dtype == torch.int32 and state.numel() >= 2
    ps = 0 if d_pos is None else _pos_stride(d_pos, B * k, pos_stride)
    if history is not None:
        assert history.dtype == torch.int64 and history.ndim == 2 and history.stride(1) == 1 and history.shape[0] == B * k
    check(L.load().mg_contrastive_finish(part.data_ptr(), n_chunk, cand_p.data_ptr(), B, k, float(alpha), hidden.data_ptr(),
                                         hidden.stride(0), d, ctx.data_ptr(), Tmax, ctx_len.data_ptr(), int(len_max), src.data_ptr(),
                                         token.data_ptr(), _p(history), 0 if history is None else history.stride(0),
                                         0 if history is None else history.shape[1], int(eos), state.data_ptr(), _p(d_pos),
                                         int(delta), ps, _stream()), "mg_contrastive_finish")


def kv_broadcast(kcache: torch.Tensor, vcache: torch.Tensor, k: int, src: torch.Tensor, d_pos: torch.Tensor, *, pos_stride: int = 0,
                 pos_delta: int = 0):
    """In every layer and head of the K / V caches [L, R, H, Smax, 256]: position ``d_pos[r] + pos_delta`` of row ``src[r // k]``
    copied to the other rows r of its group of ``k`` (mg_kv_broadcast_bf16).  One position, not kv_reorder's whole rows."""
    _need_gpu(kcache, vcache, src, d_pos)
    Lr, R, H, Smax, hd = kcache.shape
    assert hd == 256 and all(t.shape == kcache.shape and t.dtype == BF16 and t.is_contiguous() for t in (kcache, vcache))
    assert src.dtype == torch.int32 and src.is_contiguous() and src.numel() * k == R
    ps = _pos_stride(d_pos, R, pos_stride)
    check(L.load().mg_kv_broadcast_bf16(kcache.data_ptr(), vcache.data_ptr(), Lr, R, H, Smax, int(k), src.data_ptr(), d_pos.data_ptr(),
                                        ps, int(pos_delta), _stream()), "mg_kv_broadcast_bf16")


def patchify(img: torch.Tensor, P: int) -> torch.Tensor:
    """img [B,3,H,W] bf16 -> [B*(H/P)*(W/P), 3*P*P] rows in (c, py, px) order (im2col of the stride-P patch conv)."""
    _need_gpu(img)
    assert img.dtype == BF16 and img.is_contiguous() and img.ndim == 4 and img.shape[1] == 3
    B, _, H, W = img.shape
    out = torch.empty(B * (H // P) * (W // P), 3 * P * P, dtype=BF16, device=img.device)
    check(L.load().mg_patchify_bf16(img.data_ptr(), out.data_ptr(), B, H, W, P, _stream()), "mg_patchify_bf16")
    return out


def vit_embed(patches: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, B: int) -> torch.Tensor:
    """[class | patches] + positional embedding -> [B, G+1, width] bf16."""
    _need_gpu(patches, cls, pos)
    G, width = patches.shape[0] // B, patches.shape[1]
    assert patches.dtype == BF16 and cls.dtype == BF16 and pos.dtype == BF16 and pos.shape == (G + 1, width)
    out = torch.empty(B, G + 1, width, dtype=BF16, device=patches.device)
    check(L.load().mg_vit_embed_bf16(patches.data_ptr(), cls.contiguous().data_ptr(), pos.contiguous().data_ptr(), out.data_ptr(),
                                     B, G, width, _stream()), "mg_vit_embed_bf16")
    return out


def attn_small(qkv: torch.Tensor, B: int, S: int, H: int) -> torch.Tensor:
    """Non-causal attention, head dim 64, S <= 256: qkv [B*S, 3*H*64] -> [B*S, H*64]."""
    _need_gpu(qkv)
    assert qkv.dtype == BF16 and qkv.is_contiguous() and qkv.shape == (B * S, 3 * H * 64)
    out = torch.empty(B * S, H * 64, dtype=BF16, device=qkv.device)
    check(L.load().mg_attn_small_bf16(qkv.data_ptr(), out.data_ptr(), B, S, H, _stream()), "mg_attn_small_bf16")
    return out


def attn_small_bwd(qkv: torch.Tensor, d_out: torch.Tensor, B: int, S: int, H: int) -> torch.Tensor:
    """Backward of attn_small: qkv [B*S, 3*H*64], d_out [B*S, H*64] -> d_qkv [B*S, 3*H*64] (S <= 64)."""
    _need_gpu(qkv, d_out)
    assert qkv.dtype == BF16 and qkv.is_contiguous() and qkv.shape == (B * S, 3 * H * 64)
    assert d_out.dtype == BF16 and d_out.is_contiguous() and d_out.shape == (B * S, H * 64)
    dqkv = torch.empty_like(qkv)
    check(L.load().mg_attn_small_bwd_bf16(qkv.data_ptr(), d_out.data_ptr(), dqkv.data_ptr(), B, S, H, _stream()), "mg_attn_small_bwd_bf16")
    return dqkv


def avgpool2(x: torch.Tensor) -> torch.Tensor:
    """x: [B,H,W,C] NHWC bf16 contiguous."""
    _need_gpu(x)
    assert x.dtype == BF16 and x.is_contiguous() and x.ndim == 4
    B, H, W, Cc = x.shape
    y = torch.empty(B, H // 2, W // 2, Cc, dtype=BF16, device=x.device)
    check(L.load().mg_avgpool2_nhwc_bf16(x.data_ptr(), y.data_ptr(), B, H, W, Cc, _stream()), "mg_avgpool2_nhwc_bf16")
    return y


def stem_im2col(img: torch.Tensor) -> torch.Tensor:
    """img: [B,3,H,W] bf16 NCHW -> [B*(H/2)*(W/2), 32]."""
    _need_gpu(img)
    assert img.dtype == BF16 and img.is_contiguous() and img.shape[1] == 3
    B, _, H, W = img.shape
    out = torch.empty(B * (H // 2) * (W // 2), 32, dtype=BF16, device=img.device)
    check(L.load().mg_stem_im2col_bf16(img.data_ptr(), out.data_ptr(), B, H, W, _stream()), "mg_stem_im2col_bf16")
    return out


def weight_standardize(w: torch.Tensor, gain: torch.Tensor, scale: float, eps: float, to_khwc: bool = False,
                       ldo: Optional[int] = None) -> torch.Tensor:
    """timm ScaledStdConv2d weight transform: w [cout,cin,kh,kw] bf16, gain [cout(,1,1,1)] -> [cout, ldo] bf16 GEMM operand."""
    _need_gpu(w, gain)
    assert w.dtype == BF16 and gain.dtype == BF16 and w.ndim == 4 and w.is_contiguous() and gain.numel() == w.shape[0]
    cout, cin, kh, kw = w.shape
    ldo = ceil_to(cin * kh * kw, 8) if ldo is None else ldo
    out = torch.empty(cout, ldo, dtype=BF16, device=w.device)
    check(L.load().mg_weight_standardize_bf16(w.data_ptr(), gain.contiguous().data_ptr(), out.data_ptr(), cout, cin, kh, kw, ldo,
                                              int(bool(to_khwc)), float(scale), float(eps), _stream()), "mg_weight_standardize_bf16")
    return out


def im2col_nchw(img: torch.Tensor, k: int, stride: int, pad: int, ldo: int) -> torch.Tensor:
    """img [B,C,H,W] bf16 NCHW -> [B*Ho*Wo, ldo], column (c*k + ky)*k + kx (small-Cin strided stem convs)."""
    _need_gpu(img)
    assert img.dtype == BF16 and img.is_contiguous() and img.ndim == 4
    B, Cc, H, W = img.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty(B * Ho * Wo, ldo, dtype=BF16, device=img.device)
    check(L.load().mg_im2col_nchw_bf16(img.data_ptr(), out.data_ptr(), B, Cc, H, W, k, stride, pad, ldo, _stream()), "mg_im2col_nchw_bf16")
    return out


def _pool_s2(fn_name: str, x: torch.Tensor) -> torch.Tensor:
    _need_gpu(x)
    assert x.dtype == BF16 and x.is_contiguous() and x.ndim == 4
    B, H, W, Cc = x.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc, dtype=BF16, device=x.device)
    check(getattr(L.load(), fn_name)(x.data_ptr(), y.data_ptr(), B, H, W, Cc, _stream()), fn_name)
    return y


def maxpool3x3s2(x: torch.Tensor) -> torch.Tensor:
    """MaxPool2d(3, stride 2, padding 1) on [B,H,W,C] NHWC bf16."""
    return _pool_s2("mg_maxpool3x3s2_nhwc_bf16", x)


def subsample2(x: torch.Tensor) -> torch.Tensor:
    """x[:, ::2, ::2, :] of an NHWC bf16 map as a contiguous tensor."""
    return _pool_s2("mg_subsample2_nhwc_bf16", x)


def relu_mean_rows(x: torch.Tensor) -> torch.Tensor:
    """[B, HW, C] bf16 -> [B, C]: mean over the positions of relu(x)."""
    _need_gpu(x)
    assert x.dtype == BF16 and x.is_contiguous() and x.ndim == 3
    B, HW, Cc = x.shape
    y = torch.empty(B, Cc, dtype=BF16, device=x.device)
    check(L.load().mg_relu_mean_rows_bf16(x.data_ptr(), y.data_ptr(), B, HW, Cc, _stream()), "mg_relu_mean_rows_bf16")
    return y


def weight_standardize_bwd(w: torch.Tensor, gain: torch.Tensor, dwhat: torch.Tensor, dw: torch.Tensor, dgain: torch.Tensor,
                           scale: float, eps: float, dmult: float = 1.0):
    """Backward of weight_standardize: dwhat [cout, >= fan_in] fp32 (weight's own column order) -> dw [cout, fan_in] +=, dgain [cout] +=."""
    _need_gpu(w, gain, dwhat, dw, dgain)
    cout = w.shape[0]
    fan_in = w.numel() // cout
    assert w.dtype == BF16 and gain.dtype == BF16 and w.is_contiguous() and gain.numel() == cout
    assert dwhat.dtype == torch.float32 and dwhat.ndim == 2 and dwhat.stride(1) == 1 and dwhat.shape[1] >= fan_in
    assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == w.numel() and dgain.dtype == torch.float32 and dgain.numel() == cout
    check(L.load().mg_weight_standardize_bwd_f32(w.data_ptr(), gain.contiguous().data_ptr(), dwhat.data_ptr(), dwhat.stride(0), dw.data_ptr(),
                                                 dgain.data_ptr(), cout, fan_in, float(scale), float(eps), float(dmult), _stream()), "mg_weight_standardize_bwd_f32")


def maxpool3x3s2_bwd(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    _need_gpu(x, dy)
    assert x.dtype == BF16 and dy.dtype == BF16 and x.is_contiguous() and dy.is_contiguous() and x.ndim == 4
    B, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    check(L.load().mg_maxpool3x3s2_bwd_nhwc_bf16(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, H, W, Cc, _stream()), "mg_maxpool3x3s2_bwd_nhwc_bf16")
    return dx


def subsample2_bwd(dy: torch.Tensor, H: int, W: int) -> torch.Tensor:
    _need_gpu(dy)
    assert dy.dtype == BF16 and dy.is_contiguous() and dy.ndim == 4
    B, _, _, Cc = dy.shape
    dx = torch.empty(B, H, W, Cc, dtype=BF16, device=dy.device)
    check(L.load().mg_subsample2_bwd_nhwc_bf16(dy.data_ptr(), dx.data_ptr(), B, H, W, Cc, _stream()), "mg_subsample2_bwd_nhwc_bf16")
    return dx


def relu_mean_rows_bwd(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    _need_gpu(x, g)
    assert x.dtype == BF16 and g.dtype == BF16 and x.is_contiguous() and g.is_contiguous() and x.ndim == 3
    B, HW, Cc = x.shape
    dx = torch.empty_like(x)
    check(L.load().mg_relu_mean_rows_bwd_bf16(x.data_ptr(), g.data_ptr(), dx.data_ptr(), B, HW, Cc, _stream()), "mg_relu_mean_rows_bwd_bf16")
    return dx


def build_labels(captions: torch.Tensor, prefix_len: int, eos: int) -> torch.Tensor:
    _need_gpu(captions)
    assert captions.dtype == torch.int64 and captions.ndim == 2 and captions.is_contiguous()
    B, S = captions.shape
    if S < prefix_len:
        raise AssertionError("captions.shape[1] must be >= prefix length")  # reference utils.py:349
    labels = torch.empty_like(captions)
    check(L.load().mg_build_labels_i64(captions.data_ptr(), labels.data_ptr(), B, S, prefix_len, eos, _stream()),
          "mg_build_labels_i64")
    return labels


def refuse_targets_outside(targets: torch.Tensor, V: int) -> None:
    """Host-side guard of the loss paths: free where the labels are on the host (the training step), one two-element
    device-to-host copy where they are on the device (the evaluation loss, which synchronises for its row index anyway).  A label
    outside [0, V) -- a tokenizer wider than the head -- raises ValueError naming the id and V.  The kernels ignore such a target
    (cross_entropy), and the embedding gather clamps the same id (embedding), so without this it would only show as a smaller loss."""
    if targets.numel() == 0:
        return
    lo, hi = torch.stack(targets.aminmax()).tolist()          # one copy where the labels are on the device
    if hi >= V:
        raise ValueError(f"label id {hi} is outside the head's vocabulary: V = {V} (valid ids 0 .. {V - 1})")
    if lo < 0:
        raise ValueError(f"label id {lo} is negative: V = {V} (valid ids 0 .. {V - 1}; ignored positions are dropped before the loss)")


def cross_entropy(logits: torch.Tensor, targets: torch.Tensor):
    """logits [R,V] fp32 (rows already shifted), targets [R] int64.  A target of -100, or any other value outside [0, V), is
    ignored: its row loss is 0 and it is not counted in the mean (F.cross_entropy raises for such a value; no device sync here).
    Returns (mean loss scalar tensor, per-row loss); the mean is element 0 of the kernel's [mean, valid count] pair."""
    _need_gpu(logits, targets)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    assert targets.dtype == torch.int64 and targets.shape == (logits.shape[0],) and targets.is_contiguous()
    R, V = logits.shape
    rows = torch.empty(R, dtype=torch.float32, device=logits.device)
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    check(L.load().mg_ce_rows_f32(logits.data_ptr(), logits.stride(0), targets.data_ptr(), rows.data_ptr(), R, V,
                                  _stream()), "mg_ce_rows_f32")
    check(L.load().mg_ce_reduce_f32(rows.data_ptr(), targets.data_ptr(), R, V, out.data_ptr(), _stream()),
          "mg_ce_reduce_f32")
    return out[0], rows


# ======================= training path (backward + optimizer) =======================

def transpose(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[R, C] -> [C, round_up(R,8)]; the padding columns are zero (they are the K
    padding of the wgrad GEMM that consumes the result)."""
    _need_gpu(x)
    assert x.dtype == BF16 and x.ndim == 2 and x.stride(1) == 1
    R, Cc = x.shape
    if out is None:
        out = torch.empty(Cc, ceil_to(R, 8), dtype=BF16, device=x.device)
    check(L.load().mg_transpose_bf16(x.data_ptr(), x.stride(0), 0, out.data_ptr(), out.stride(0), 0, R, Cc, 1, _stream()),
          "mg_transpose_bf16")
    return out


def transpose_colsum(x: torch.Tensor, colsum_out: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """transpose(x) that also accumulates the column sums of x into colsum_out (fp32 [C]): one pass instead of two.
    ``out`` as for ``transpose``: [C, round_up(R, 8)] bf16, any row stride."""
    _need_gpu(x, colsum_out, out)
    assert x.dtype == BF16 and x.ndim == 2 and x.stride(1) == 1 and colsum_out.dtype == torch.float32 and colsum_out.numel() >= x.shape[1]
    R, Cc = x.shape
    if out is None:
        out = torch.empty(Cc, ceil_to(R, 8), dtype=BF16, device=x.device)
    assert out.dtype == BF16 and out.ndim == 2 and out.stride(1) == 1 and tuple(out.shape) == (Cc, ceil_to(R, 8))
    check(L.load().mg_transpose_colsum_bf16(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), R, Cc, colsum_out.data_ptr(), _stream()),
          "mg_transpose_colsum_bf16")
    return out


def head_transpose(src: torch.Tensor, B: int, H: int, S: int, sb: int, ss: int, sh: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> column-tiled transposed layout [B, H, ceil(S/32), 256, 32]: out[b,h,t,d,i] = src[b, 32t+i, h, d], zero padded."""
    _need_gpu(src)
    ld = ceil_to(S, 32)
    if out is None:
        out = torch.empty(B, H, ld // 32, 256, 32, dtype=BF16, device=src.device)
    check(L.load().mg_head_transpose_bf16(src.data_ptr(), sb, ss, sh, out.data_ptr(), ld, B, H, S, _stream()),
          "mg_head_transpose_bf16")
    return out


def colsum(x: torch.Tensor, out: torch.Tensor, y: Optional[torch.Tensor] = None, deterministic: bool = False):
    """out[n] += sum_m x[m,n] * (y[m,n] if y else 1); out fp32 [N].  deterministic: partials per 256 rows added in row order by a
    second launch instead of fp32 atomics -- the same bits in every run (for sums that feed a rounding decision)."""
    _need_gpu(x, out)
    assert x.dtype == BF16 and x.ndim == 2 and x.stride(1) == 1 and out.dtype == torch.float32
    if deterministic:
        parts = torch.empty(L.load().mg_colsum_det_parts(x.shape[0]), x.shape[1], dtype=torch.float32, device=x.device)
        check(L.load().mg_colsum_det_f32(x.data_ptr(), x.stride(0), _p(y), 0 if y is None else y.stride(0), out.data_ptr(),
                                         parts.data_ptr(), x.shape[0], x.shape[1], _stream()), "mg_colsum_det_f32")
        return out
    check(L.load().mg_colsum_f32(x.data_ptr(), x.stride(0), _p(y), 0 if y is None else y.stride(0), out.data_ptr(),
                                 x.shape[0], x.shape[1], _stream()), "mg_colsum_f32")
    return out


def layernorm_bwd(dy, x, gamma, eps=1e-5, res=None, want_xhat=False):
    _need_gpu(dy, x)
    assert dy.dtype == BF16 and x.dtype == BF16 and x.ndim == 2 and dy.shape == x.shape and dy.stride(1) == 1 and x.stride(1) == 1
    _need_gpu(gamma, res)
    assert gamma.dtype == torch.float32 and gamma.shape == (x.shape[1],) and gamma.is_contiguous(), "gamma: fp32 [d]"
    assert res is None or (res.dtype == BF16 and res.shape == x.shape and res.stride(1) == 1), "res: bf16, x's shape, unit inner stride"
    dx = torch.empty(x.shape, dtype=BF16, device=x.device)
    xhat = torch.empty(x.shape, dtype=BF16, device=x.device) if want_xhat else None
    check(L.load().mg_layernorm_bwd_bf16(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), gamma.data_ptr(),
                                         _p(res), 0 if res is None else res.stride(0), dx.data_ptr(), dx.stride(0),
                                         _p(xhat), 0 if xhat is None else xhat.stride(0), x.shape[0], x.shape[1], eps,
                                         _stream()), "mg_layernorm_bwd_bf16")
    return (dx, xhat) if want_xhat else dx


def cross_entropy_fwd_bwd(logits: torch.Tensor, targets: torch.Tensor, ld_out: int):
    """loss + dlogits (bf16 [R, ld_out], columns [V, ld_out) zero) for rows already shifted; targets as in cross_entropy: a row
    whose target is -100 or outside [0, V) has gradient 0 and is not counted in the 1 / n of the others."""
    _need_gpu(logits, targets)
    assert logits.dtype == torch.float32 and logits.ndim == 2 and logits.stride(1) == 1
    assert targets.dtype == torch.int64 and targets.shape == (logits.shape[0],) and targets.is_contiguous()
    assert ld_out >= logits.shape[1], "ld_out < V"
    R, V = logits.shape
    rows = torch.empty(R, dtype=torch.float32, device=logits.device)
    stats = torch.empty(2, dtype=torch.float32, device=logits.device)
    lib = L.load()
    check(lib.mg_ce_rows_f32(logits.data_ptr(), logits.stride(0), targets.data_ptr(), rows.data_ptr(), R, V, _stream()), "mg_ce_rows_f32")
    check(lib.mg_ce_reduce_f32(rows.data_ptr(), targets.data_ptr(), R, V, stats.data_ptr(), _stream()), "mg_ce_reduce_f32")
    dl = torch.empty(R, ld_out, dtype=BF16, device=logits.device)
    check(lib.mg_ce_bwd_bf16(logits.data_ptr(), logits.stride(0), targets.data_ptr(), stats.data_ptr(), dl.data_ptr(),
                             ld_out, R, V, _stream()), "mg_ce_bwd_bf16")
    return stats[0], dl


MG_ACT_GELU_ERF = 100      # NOT an epilogue code: torch.nn.GELU() runs as its own pass (gelu_erf / gelu_erf_grad_mul below)
MG_AUX_GELU_ERF_GRAD = 100


def gelu_erf(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch.nn.GELU() (erf) over a [rows, cols] bf16 matrix (row stride allowed); ``out`` may be x."""
    _need_gpu(x)
    assert x.dtype == BF16 and x.ndim == 2 and x.stride(1) == 1 and x.shape[1] % 8 == 0
    if out is None:
        out = torch.empty_like(x)
    check(L.load().mg_gelu_erf_bf16(x.data_ptr(), x.stride(0), None, 0, out.data_ptr(), out.stride(0), x.shape[0], x.shape[1], _stream()),
          "mg_gelu_erf_bf16")
    return out


def gelu_erf_grad_mul(g: torch.Tensor, pre: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g * gelu'(pre) (erf form), same shapes; ``out`` may be g."""
    _need_gpu(g, pre)
    assert g.dtype == BF16 and pre.dtype == BF16 and g.shape == pre.shape and g.stride(1) == 1 and pre.stride(1) == 1 and g.shape[1] % 8 == 0
    if out is None:
        out = torch.empty_like(g)
    check(L.load().mg_gelu_erf_bf16(pre.data_ptr(), pre.stride(0), g.data_ptr(), g.stride(0), out.data_ptr(), out.stride(0),
                                    g.shape[0], g.shape[1], _stream()), "mg_gelu_erf_bf16")
    return out


def rotary_merge_bwd(dq, dk, dv, B, S, H, rot_dim, sin_t, cos_t):
    _need_gpu(dq)
    out = torch.empty(B * S, 3 * H * 256, dtype=BF16, device=dq.device)
    check(L.load().mg_rotary_merge_bwd_bf16(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, S, H, rot_dim,
                                            sin_t.data_ptr(), cos_t.data_ptr(), out.data_ptr(), _stream()),
          "mg_rotary_merge_bwd_bf16")
    return out


def attn_bwd(q, k, v, qt, kt, dO, dOt, O, lse, B, H, S):
    """q,k,v [B,H,S,256]; qt,kt,dOt [B,H,256,ld]; dO [B*S,H*256]; O [B*S, >= H*256] (any row stride); lse [B,H,S]
    -> dq,dk,dv [B,H,S,256]."""
    _need_gpu(q)
    assert O.ndim == 2 and O.stride(1) == 1 and dO.is_contiguous()
    dev = q.device
    D = torch.empty(B, H, S, 2, dtype=torch.float32, device=dev)   # {-16 lse, -rowsum(dO o O)} per query (workspace)
    dq, dk, dv = (torch.empty(B, H, S, 256, dtype=BF16, device=dev) for _ in range(3))
    check(L.load().mg_attn_bwd_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), qt.data_ptr(), kt.data_ptr(),
                                    dO.data_ptr(), dOt.data_ptr(), O.data_ptr(), lse.data_ptr(), D.data_ptr(),
                                    dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, H, S, qt.shape[2] * 32, O.stride(0), _stream()),
          "mg_attn_bwd_bf16")
    return dq, dk, dv


def attn_bwd_merged(q, k, v, qt, kt, dO, O, lse, B, H, S, rot_dim, sin_t, cos_t, out=None):
    """dO transpose + attn_bwd + rotary_merge_bwd in one call: -> dqkv [B*S, 3*H*256] (gradient of the fused qkv
    projection).  ``out``: a contiguous bf16 [B*S, 3*H*256] to write into instead of a new tensor."""
    _need_gpu(q)
    assert O.ndim == 2 and O.stride(1) == 1 and dO.is_contiguous()       # O may be the [:, :d] view of a [ctx | t] buffer
    dev = q.device
    D = torch.empty(B, H, S, 2, dtype=torch.float32, device=dev)
    dOt = torch.empty_like(qt)                                       # workspace, filled by the first launch
    dqkv = _grad_out(out, (B * S, 3 * H * 256), dev)
    check(L.load().mg_attn_bwd_merged_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), qt.data_ptr(), kt.data_ptr(),
                                           dO.data_ptr(), dOt.data_ptr(), O.data_ptr(), lse.data_ptr(), D.data_ptr(),
                                           dqkv.data_ptr(), rot_dim, sin_t.data_ptr(), cos_t.data_ptr(), B, H, S,
                                           qt.shape[2] * 32, O.stride(0), _stream()), "mg_attn_bwd_merged_bf16")
    return dqkv


class AttnRows:
    """q / k / v of a batch of heads as strided rows of 256 (include/magma_hip.h, attention without transposed images): either three
    [B,H,S,256] tensors or -- ``AttnRows.of_qkv`` -- column ranges of the fused qkv activation [B*S, 3 H 256] itself."""

    def __init__(self, q, k, v, ld_row, stride_b, stride_h, B, H, S, keep=()):
        self.q, self.k, self.v, self.ld_row, self.stride_b, self.stride_h = q, k, v, ld_row, stride_b, stride_h
        self.B, self.H, self.S, self.keep = B, H, S, keep          # keep: the tensors the pointers live in

    @classmethod
    def of_bhsd(cls, q, k, v):
        B, H, S, dh = q.shape
        assert dh == 256 and q.is_contiguous() and k.is_contiguous() and v.is_contiguous() and k.shape == q.shape == v.shape
        return cls(q.data_ptr(), k.data_ptr(), v.data_ptr(), 256, H * S * 256, S * 256, B, H, S, keep=(q, k, v))

    @classmethod
    def of_qkv(cls, qkv, B, S, H):
        assert qkv.ndim == 2 and qkv.stride(1) == 1 and qkv.shape[0] == B * S and qkv.shape[1] >= 3 * H * 256
        ld, p = qkv.stride(0), qkv.data_ptr()
        return cls(p, p + H * 256 * 2, p + 2 * H * 256 * 2, ld, S * ld, 256, B, H, S, keep=(qkv,))


def rotary_qk_inplace(qkv, B, S, H, rot_dim, sin_t, cos_t):
    """GPT-J rotary on the q and k sections of qkv [B*S, >= 3 H 256], in place (v untouched)."""
    _need_gpu(qkv)
    assert qkv.ndim == 2 and qkv.stride(1) == 1 and qkv.shape[0] == B * S
    check(L.load().mg_rotary_qk_inplace_bf16(qkv.data_ptr(), qkv.stride(0), B, S, H, rot_dim, sin_t.data_ptr(), cos_t.data_ptr(),
                                             _stream()), "mg_rotary_qk_inplace_bf16")
    return qkv


def attn_fwd_rows(x: AttnRows, out, lse: Optional[torch.Tensor] = None):
    """Causal flash attention reading q / k / v as strided rows (no V^T): out [B*S, >= H*256] (a column range of a wider row is fine)."""
    _need_gpu(out)
    assert out.ndim == 2 and out.stride(1) == 1 and out.shape[1] == x.H * 256
    check(L.load().mg_attn_fwd_rows_bf16(x.q, x.k, x.v, x.ld_row, x.stride_b, x.stride_h, out.data_ptr(), out.stride(0), _p(lse),
                                         x.B, x.H, x.S, _stream()), "mg_attn_fwd_rows_bf16")
    return out


def _grad_out(out, shape, dev):
    """A gradient output of the attention backward: new, or the caller's ``out`` (contiguous bf16 of that shape)."""
    if out is None:
        return torch.empty(shape, dtype=BF16, device=dev)
    _need_gpu(out)
    assert out.dtype == BF16 and tuple(out.shape) == tuple(shape) and out.is_contiguous(), f"out: contiguous bf16 {tuple(shape)}"
    return out


def attn_bwd_rows(x: AttnRows, dO, O, lse, merged_rot=None, mx_out=None, no_out: bool = False, first_rows: int = 0, out=None):
    """Attention backward without transposed operands.  merged_rot None -> (dq, dk, dv) [B,H,S,256]; merged_rot = (rot_dim, sin_t,
    cos_t) -> dqkv [B*S, 3 H 256], the gradient of the fused qkv projection (inverse rotary applied).  Merged form only:
    ``mx_out`` = (q, scales) from mx_empty(B*S, 3 H 256) -> the epilogue also writes the OCP MX e4m3 copy of dqkv; with ``no_out``
    only that copy (returns None).  ``first_rows`` > 0: only the gradients of the positions < first_rows of every sequence are
    wanted (rounded up to whole 128-position blocks; the other rows of the outputs stay unwritten).  ``out``: the tensor(s) to
    write into instead of new ones -- (dq, dk, dv) for the separate form, dqkv for the merged one."""
    _need_gpu(dO)
    assert O.ndim == 2 and O.stride(1) == 1 and dO.is_contiguous()
    # the rows first_rows leaves unwritten would keep 0xFF scale bytes (NaN in E8M0) in an MX copy read in whole 64-row groups
    assert not (first_rows and mx_out is not None), "first_rows and mx_out exclude each other"
    B, H, S, dev = x.B, x.H, x.S, dO.device
    D = torch.empty(B, H, S, 2, dtype=torch.float32, device=dev)
    if merged_rot is None:
        dq, dk, dv = (_grad_out(t, (B, H, S, 256), dev) for t in (out if out is not None else (None, None, None)))
        check(L.load().mg_attn_bwd_rows_bf16(x.q, x.k, x.v, x.ld_row, x.stride_b, x.stride_h, dO.data_ptr(), O.data_ptr(), O.stride(0),
                                             lse.data_ptr(), D.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), None, 0, None, None,
                                             B, H, S, None, None, int(first_rows), _stream()), "mg_attn_bwd_rows_bf16")
        return dq, dk, dv
    rot_dim, sin_t, cos_t = merged_rot
    q8, sc8 = mx_out if mx_out is not None else (None, None)
    assert not no_out or q8 is not None
    if q8 is not None:
        assert q8.dtype == torch.uint8 and q8.shape[0] >= B * S and q8.stride(0) == 3 * H * 256
        assert sc8.numel() == int(L.load().mg_mx_scale_bytes(B * S, 3 * H * 256))
    assert not (no_out and out is not None), "no_out and out exclude each other"
    dqkv = None if no_out else _grad_out(out, (B * S, 3 * H * 256), dev)
    check(L.load().mg_attn_bwd_rows_bf16(x.q, x.k, x.v, x.ld_row, x.stride_b, x.stride_h, dO.data_ptr(), O.data_ptr(), O.stride(0),
                                         lse.data_ptr(), D.data_ptr(), None, None, None, _p(dqkv), rot_dim, sin_t.data_ptr(),
                                         cos_t.data_ptr(), B, H, S, _p(q8), _p(sc8), int(first_rows), _stream()), "mg_attn_bwd_rows_bf16")
    return dqkv


def avgpool2_bwd(dy: torch.Tensor, B, H, W, Cc, gate: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dy [B,H/2,W/2,C] -> dx [B,H,W,C] (zeroed where gate <= 0 when a gate is given)."""
    _need_gpu(dy)
    dx = torch.empty(B, H, W, Cc, dtype=BF16, device=dy.device)
    check(L.load().mg_avgpool2_bwd_nhwc_bf16(dy.data_ptr(), _p(gate), dx.data_ptr(), B, H, W, Cc, _stream()), "mg_avgpool2_bwd_nhwc_bf16")
    return dx


def mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _need_gpu(a, b)
    out = torch.empty_like(a)
    check(L.load().mg_mul_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "mg_mul_bf16")
    return out


def scale_rows_acc(dst: torch.Tensor, src: torch.Tensor, row_scale: Optional[torch.Tensor] = None):
    """dst[r,c] += src[r,c] * row_scale[r]; dst fp32 contiguous view of a flat gradient buffer."""
    _need_gpu(dst, src)
    assert dst.dtype == torch.float32 and src.dtype == torch.float32 and src.stride(1) == 1 and dst.is_contiguous()
    rows, cols = dst.shape
    check(L.load().mg_scale_rows_acc_f32(dst.data_ptr(), src.data_ptr(), src.stride(0), _p(row_scale), rows, cols, _stream()),
          "mg_scale_rows_acc_f32")


def scale_rows_acc_bn_grad(dst, src, w, row_scale, mean, var, eps, gsum, dgamma, dbeta):
    """The parameter gradients of a conv + frozen-statistics BatchNorm unit from the unscaled product src = g^T a (fp32 [Cout, >= K],
    any row stride), the bf16 weight w [Cout, K] and gsum = the column sums of g:
    dst[r,c] += src[r,c] * row_scale[r];  dbeta += gsum;  dgamma[r] += rsqrt(var[r] + eps) * (<src[r], w[r]> - mean[r] * gsum[r]).
    <src[r], w[r]> = sum_m g[m,r] z[m,r] with z the convolution output, which the forward never stores."""
    _need_gpu(dst, src, w, row_scale, mean, var, gsum, dgamma, dbeta)
    rows, cols = dst.shape
    assert dst.dtype == torch.float32 and dst.is_contiguous() and src.dtype == torch.float32 and src.stride(1) == 1
    assert src.shape[0] == rows and src.shape[1] >= cols and w.dtype == BF16 and w.is_contiguous() and tuple(w.shape) == (rows, cols)
    for t in (row_scale, mean, var, gsum, dgamma, dbeta):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == rows
    check(L.load().mg_scale_rows_acc_bn_grad_f32(dst.data_ptr(), src.data_ptr(), src.stride(0), w.data_ptr(), row_scale.data_ptr(),
                                                 mean.data_ptr(), var.data_ptr(), float(eps), gsum.data_ptr(), dgamma.data_ptr(),
                                                 dbeta.data_ptr(), rows, cols, _stream()), "mg_scale_rows_acc_bn_grad_f32")


def add_gate(a, b=None, gate=None, out=None):
    """out = (a + b) * (gate > 0); b, gate optional; flat bf16 tensors of equal numel (multiple of 8)."""
    _need_gpu(a)
    if out is None:
        out = torch.empty_like(a)
    check(L.load().mg_add_gate_bf16(a.data_ptr(), _p(b), _p(gate), out.data_ptr(), a.numel(), _stream()), "mg_add_gate_bf16")
    return out


def bn_param_grad(g, y, sub, gamma, beta, dgamma, dbeta):
    _need_gpu(g)
    M, Cc = g.shape
    check(L.load().mg_bn_param_grad_f32(g.data_ptr(), y.data_ptr(), _p(sub), gamma.data_ptr(), beta.data_ptr(),
                                        dgamma.data_ptr(), dbeta.data_ptr(), M, Cc, _stream()), "mg_bn_param_grad_f32")


def transpose_bn_param_grad(g, y, sub, gamma, beta, dgamma, dbeta) -> torch.Tensor:
    """g^T [C, round_up(M, 8)] (as ``transpose``) and, from the same pass over g, the frozen-statistics BatchNorm parameter gradients
    that ``bn_param_grad`` accumulates."""
    _need_gpu(g, y, sub, gamma, beta, dgamma, dbeta)
    M, Cc = g.shape
    assert g.dtype == BF16 and g.stride(1) == 1 and y.shape == g.shape and y.stride() == g.stride() and (sub is None or (sub.shape == g.shape and sub.stride() == g.stride()))
    out = torch.empty(Cc, ceil_to(M, 8), dtype=BF16, device=g.device)
    check(L.load().mg_transpose_bn_param_grad_bf16(g.data_ptr(), g.stride(0), out.data_ptr(), out.stride(0), M, Cc, y.data_ptr(), _p(sub),
                                                   gamma.data_ptr(), beta.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), _stream()),
          "mg_transpose_bn_param_grad_bf16")
    return out


def im2col_t(x_nhwc: torch.Tensor, B, H, W, Cin) -> torch.Tensor:
    """-> [Cin*9, round_up(M,8)] (row = ci*9 + tap, zero padded columns) for the 3x3 wgrad GEMM."""
    _need_gpu(x_nhwc)
    M = B * H * W
    ldo = ceil_to(M, 8)
    out = torch.empty(9 * Cin, ldo, dtype=BF16, device=x_nhwc.device)
    check(L.load().mg_im2col_t_bf16(x_nhwc.data_ptr(), out.data_ptr(), ldo, B, H, W, Cin, _stream()), "mg_im2col_t_bf16")
    return out


def sumsq(g: torch.Tensor, out: torch.Tensor):
    """out[0] += sum(g^2); g fp32 or bf16 (the exchanged buckets of the data-parallel step)."""
    _need_gpu(g, out)
    fn = L.load().mg_sumsq_bf16 if g.dtype == BF16 else L.load().mg_sumsq_f32
    check(fn(g.data_ptr(), g.numel(), out.data_ptr(), _stream()), "mg_sumsq")


def cast_f32_bf16(src: torch.Tensor, dst: torch.Tensor):
    _need_gpu(src, dst)
    assert src.dtype == torch.float32 and dst.dtype == BF16 and src.numel() == dst.numel() and src.is_contiguous()
    check(L.load().mg_cast_f32_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), _stream()), "mg_cast_f32_bf16")
    return dst


def adamw(p, m, v, g, p_bf16, lr, beta1, beta2, eps, wd, step, max_norm=0.0, norm_sq=None, grad_scale=1.0):
    """Fused clip + AdamW on fp32 master / m / v; g = gradient sum in fp32 or bf16."""
    _need_gpu(p, g)
    fn = L.load().mg_adamw_gbf16_f32 if g.dtype == BF16 else L.load().mg_adamw_f32
    check(fn(p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), _p(p_bf16), p.numel(), lr,
             beta1, beta2, eps, wd, step, max_norm, _p(norm_sq), grad_scale, _stream()), "mg_adamw")


def bn_fold(gamma, beta, mean, var, eps: float):
    """(scale, shift) fp32 [C] of a frozen-statistics BatchNorm: scale = gamma / sqrt(var + eps), shift = beta - mean*scale."""
    _need_gpu(gamma)
    for t in (gamma, beta, mean, var):
        assert t.dtype == torch.float32 and t.is_contiguous()
    scale, shift = torch.empty_like(gamma), torch.empty_like(gamma)
    check(L.load().mg_bn_fold_f32(gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), eps, scale.data_ptr(),
                                  shift.data_ptr(), gamma.numel(), _stream()), "mg_bn_fold_f32")
    return scale, shift


def bn_batch_fold(s1, s2, gamma, beta, M: int, eps: float, momentum: float, running_mean=None, running_var=None):
    """Per-channel batch statistics -> (scale, shift, mean, rstd) fp32 [C]; running statistics updated in place (fp32 tensors)."""
    _need_gpu(s1, s2, gamma, beta)
    C_ = s1.numel()
    scale, shift, mean, rstd = (torch.empty(C_, dtype=torch.float32, device=s1.device) for _ in range(4))
    check(L.load().mg_bn_batch_fold_f32(s1.data_ptr(), s2.data_ptr(), gamma.data_ptr(), beta.data_ptr(), M, eps, momentum,
                                        _p(running_mean), _p(running_var), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                                        rstd.data_ptr(), C_, _stream()), "mg_bn_batch_fold_f32")
    return scale, shift, mean, rstd


def bn_apply(z, scale, shift, res=None, relu=True):
    _need_gpu(z, res)
    assert z.dtype == BF16 and z.ndim == 2 and z.is_contiguous()
    y = torch.empty_like(z)
    check(L.load().mg_bn_apply_bf16(z.data_ptr(), scale.data_ptr(), shift.data_ptr(), _p(res), int(bool(relu)), y.data_ptr(),
                                    z.shape[0], z.shape[1], _stream()), "mg_bn_apply_bf16")
    return y


def bn_bwd_dz(g, z, mean, rstd, gamma, dgamma, dbeta):
    _need_gpu(g, z)
    assert g.dtype == BF16 and z.dtype == BF16 and g.shape == z.shape and g.is_contiguous() and z.is_contiguous()
    dz = torch.empty_like(z)
    check(L.load().mg_bn_bwd_dz_bf16(g.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                     dgamma.data_ptr(), dbeta.data_ptr(), dz.data_ptr(), z.shape[0], z.shape[1], _stream()),
          "mg_bn_bwd_dz_bf16")
    return dz


def conv_weight_relayout(w: torch.Tensor, mode: int, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[Cout, Cin, k, k] bf16 conv weight -> row-major GEMM operand with K zero padded to a multiple of 64.
    mode 0: [Cout, k*k*Cin] in (ky, kx, ci) order; mode 1: [Cin, k*k*Cout] with flipped taps times scale[co] (dgrad)."""
    _need_gpu(w)
    assert w.dtype == BF16 and w.ndim == 4 and w.is_contiguous() and w.shape[2] == w.shape[3]
    cout, cin, k, _ = w.shape
    rows, inner = (cout, cin) if mode == 0 else (cin, cout)
    ldo = ceil_to(k * k * inner, 64)
    out = torch.empty(rows, ldo, dtype=BF16, device=w.device)
    check(L.load().mg_conv_weight_relayout_bf16(w.data_ptr(), _p(scale), out.data_ptr(), ldo, cout, cin, k, mode, _stream()),
          "mg_conv_weight_relayout_bf16")
    return out


def _job_table(jobs, device) -> torch.Tensor:
    """ctypes job structs -> device byte tensor (the DEVICE array the batched entry points read)."""
    arr = (type(jobs[0]) * len(jobs))(*jobs)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


class ConvOperandPlan:
    """GEMM operands of MANY trainable convolutions + the folded affine of their frozen-statistics BatchNorms, re-derived from the
    current weights by TWO launches (mg_bn_fold_batch, then mg_conv_weight_relayout_batch) -- the training engine calls ``refresh``
    once per forward instead of ~3 small launches per convolution.  ``units``: list of (weight bf16 [Cout,Cin,k,k] with k in (1, 3),
    gamma, beta, mean, var fp32 [Cout], eps); weight / statistics storage must stay where it is (the tables hold raw pointers).
    Per unit i afterwards: ``fwd[i]`` [Cout, ld] (mode 0), ``dgrad[i]`` [Cin, ld] (mode 1, BN scale folded), ``scale[i]``, ``shift[i]``."""

    def __init__(self, units, device):
        from .lib import BnFoldJob, RelayoutJob
        self.keep = units
        ctot = sum(u[0].shape[0] for u in units)
        self._aff = torch.empty(2, ctot, dtype=torch.float32, device=device)
        self.scale, self.shift, self.fwd, self.dgrad = [], [], [], []
        sizes = []
        for (w, *_rest) in units:
            _need_gpu(w)
            assert w.dtype == BF16 and w.ndim == 4 and w.is_contiguous() and w.shape[2] == w.shape[3] and w.shape[2] in (1, 3)
            cout, cin, k, _ = w.shape
            # (a 1x1 weight whose Cin is a whole number of 64-element K-tiles already IS its forward operand: no copy)
            sizes.append((0 if (k == 1 and cin % 64 == 0) else cout * ceil_to(k * k * cin, 64), cin * ceil_to(k * k * cout, 64)))
        self._ops = torch.empty(sum(a + b for a, b in sizes), dtype=BF16, device=device)
        bn_jobs, rl_jobs, c0, o0, bb, rb = [], [], 0, 0, 0, 0
        for (w, gamma, beta, mean, var, eps), (n0, n1) in zip(units, sizes):
            cout, cin, k, _ = w.shape
            for t in (gamma, beta, mean, var):
                _need_gpu(t)
                assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == cout
            sc, sh = self._aff[0, c0:c0 + cout], self._aff[1, c0:c0 + cout]
            c0 += cout
            bn_jobs.append(BnFoldJob(gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                     float(eps), cout, bb))
            bb += (cout + 255) // 256
            g = self._ops[o0 + n0:o0 + n0 + n1].view(cin, -1)
            if n0:
                f = self._ops[o0:o0 + n0].view(cout, -1)
                rl_jobs.append(RelayoutJob(w.data_ptr(), None, f.data_ptr(), f.shape[1], cout, cin, k, 0, rb))
                rb += (n0 + 255) // 256
            else:
                f = w.view(cout, cin)
            o0 += n0 + n1
            rl_jobs.append(RelayoutJob(w.data_ptr(), sc.data_ptr(), g.data_ptr(), g.shape[1], cout, cin, k, 1, rb))
            rb += (n1 + 255) // 256
            self.scale.append(sc); self.shift.append(sh); self.fwd.append(f); self.dgrad.append(g)
        self._bn_tab, self._rl_tab = _job_table(bn_jobs, device), _job_table(rl_jobs, device)
        self._nbn, self._bn_blocks, self._nrl, self._rl_blocks = len(bn_jobs), bb, len(rl_jobs), rb

    def refresh(self):
        lib = L.load()
        check(lib.mg_bn_fold_batch(self._bn_tab.data_ptr(), self._nbn, self._bn_blocks, _stream()), "mg_bn_fold_batch")
        check(lib.mg_conv_weight_relayout_batch(self._rl_tab.data_ptr(), self._nrl, self._rl_blocks, _stream()), "mg_conv_weight_relayout_batch")


# ---- image preprocessing (reference magma/transforms.py:121-134) ------------------------------------------------
def resample_u8(img: torch.Tensor, out_size: int, axis: int, coeffs: torch.Tensor, bounds: torch.Tensor) -> torch.Tensor:
    """One pass of Pillow's 8-bit antialiased resampling on an HWC uint8 RGB image (axis 1: width, axis 0: height)."""
    _need_gpu(img)
    assert img.dtype == torch.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.is_contiguous()
    assert coeffs.dtype == torch.int32 and bounds.dtype == torch.int32 and coeffs.is_contiguous() and bounds.is_contiguous()
    H, W, _ = img.shape
    out = torch.empty((H, out_size, 3) if axis == 1 else (out_size, W, 3), dtype=torch.uint8, device=img.device)
    check(L.load().mg_resample_u8(img.data_ptr(), H, W, out.data_ptr(), out_size, axis, coeffs.data_ptr(), bounds.data_ptr(),
                                  coeffs.shape[1], _stream()), "mg_resample_u8")
    return out


def crop_normalize(img: torch.Tensor, top: int, left: int, n: int, mean, std) -> torch.Tensor:
    """HWC uint8 -> [3, n, n] fp32, (v / 255 - mean) / std  (CenterCrop + ToTensor + Normalize)."""
    _need_gpu(img)
    assert img.dtype == torch.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.is_contiguous()
    out = torch.empty(3, n, n, dtype=torch.float32, device=img.device)
    m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    check(L.load().mg_crop_normalize_f32(img.data_ptr(), img.shape[0], img.shape[1], top, left, n, m3, s3, out.data_ptr(), _stream()),
          "mg_crop_normalize_f32")
    return out


# ---- fp8 (OCP e4m3) GEMM operands: BASELINE config 5 ---------------------------------------------------------------
def quantize_rows_fp8(x: torch.Tensor, ldq: Optional[int] = None):
    """bf16 [M, K] -> (uint8 e4m3 [M, ldq] zero padded, fp32 row scales [M]);  x ~= q * scale[:, None]."""
    _need_gpu(x)
    assert x.dtype == BF16 and x.ndim == 2 and x.stride(1) == 1
    M, K = x.shape
    ldq = ceil_to(K, 128) if ldq is None else ldq
    q = torch.empty(M, ldq, dtype=torch.uint8, device=x.device)
    scale = torch.empty(M, dtype=torch.float32, device=x.device)
    check(L.load().mg_quantize_rows_fp8(x.data_ptr(), x.stride(0), M, K, q.data_ptr(), ldq, scale.data_ptr(), _stream()),
          "mg_quantize_rows_fp8")
    return q, scale


class PackedLinearFP8:
    """A [N, K] weight as e4m3 bytes with one fp32 scale per output channel (W ~= q * scale[:, None]), in the same two
    layouts as PackedLinear: row-major [N, Kp] and fragment-tiled (the bf16 tiling applied to byte PAIRS, Kp % 128 == 0)."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, tiled: bool = True, rowmajor: bool = False):
        _need_gpu(weight)
        self.N, self.K = weight.shape
        assert self.K % 16 == 0, "fp8 GEMM needs K % 16 == 0"
        self.Kp = ceil_to(self.K, 128)
        n16 = ceil_to(self.N, 16)
        w = torch.zeros(n16, self.K, dtype=BF16, device=weight.device)
        w[: self.N] = weight.detach().to(BF16)
        q, sc = quantize_rows_fp8(w, self.Kp)
        self.scale = sc[: self.N].contiguous()
        self.bias = None if bias is None else bias.detach().to(torch.float32).contiguous()
        self.rm = q[: self.N].contiguous() if rowmajor else None
        self.ft = PackedLinear.tile(q.view(torch.int16)).view(torch.uint8) if tiled else None   # pairs of bytes tile like bf16

    def dequant(self) -> torch.Tensor:
        q = self.rm if self.rm is not None else PackedLinear.untile(self.ft.view(torch.int16)).view(torch.uint8)[: self.N]
        return q[:, : self.K].view(torch.float8_e4m3fn).float() * self.scale[:, None]

    @classmethod
    def of_live(cls, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> "PackedLinearFP8":
        """The fragment-tiled pack of a TRAINABLE [N, K] bf16 weight (N % 16 == 0, K % 128 == 0), rebuilt every optimizer step: two
        launches (quantise, tile), no padding copies; ``bias`` is kept by reference (a live fp32 master view)."""
        self = cls.__new__(cls)
        self.N, self.K = weight.shape
        assert weight.dtype == BF16 and weight.stride(1) == 1 and self.N % 16 == 0 and self.K % 128 == 0
        self.Kp = self.K
        q, self.scale = quantize_rows_fp8(weight, self.Kp)
        self.bias, self.rm = bias, None
        self.ft = PackedLinear.tile(q.view(torch.int16)).view(torch.uint8)
        return self


def gemm_fp8(aq: torch.Tensor, a_scale: torch.Tensor, w: PackedLinearFP8, out: Optional[torch.Tensor] = None, *,
             act: int = MG_ACT_NONE, residuals: Sequence[torch.Tensor] = (), act_after: int = MG_ACT_NONE,
             use_bias: bool = True, out_dtype=BF16, layout: Optional[str] = None, split_k: int = 0,
             aux=None, aux_mode: int = MG_AUX_NONE, aux_after: bool = False, out2: Optional[torch.Tensor] = None,
             tile: int = 0, mx_out=None, no_out: bool = False):
    """out[M,N] = epilogue((aq @ wq^T) * a_scale[m] * w.scale[n]) on the fp8 MFMA (fp32 accumulate).
    ``tile``: 0 lets the library choose between the 128x128 and the 256x256 kernel, 128 / 256 force one.
    ``mx_out`` (from mx_empty): the epilogue also writes the MX e4m3 copy of the result; with ``no_out`` only that copy
    (returns None)."""
    _need_gpu(aq)
    assert aq.dtype == torch.uint8 and aq.ndim == 2 and aq.stride(1) == 1 and aq.shape[1] >= w.K
    M = aq.shape[0]
    assert not no_out or (mx_out is not None and out is None)
    if out is None and not no_out:
        out = torch.empty(M, ceil_to(w.N, 8), dtype=out_dtype, device=aq.device)[:, : w.N]
    d = GemmDesc()
    d.A, d.lda = aq.data_ptr(), aq.stride(0)
    if layout is None:
        layout = "ft" if w.ft is not None else "rm"
    if layout == "ft":
        d.W, d.ldw, d.w_layout = w.ft.data_ptr(), w.Kp, MG_W_FRAGTILED
    else:
        d.W, d.ldw, d.w_layout = w.rm.data_ptr(), w.rm.stride(0), MG_W_ROWMAJOR
    d.M, d.N, d.K = M, w.N, w.K
    d.a_mode = MG_A_DENSE
    d.tile_hint = tile
    d.zero_page = zero_page(aq.device).data_ptr()
    d.split_k = split_k
    if split_k != 1:
        ws = splitk_workspace(aq.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    d.ep = _epilogue(out, w.N, w.bias if use_bias else None, w.scale, act, residuals, act_after, aux, aux_mode, aux_after, out2,
                     mx_out=mx_out, M=M)
    check(L.load().mg_gemm_fp8(C.byref(d), a_scale.data_ptr(), _stream()), "mg_gemm_fp8")
    return out


# ---- OCP MX fp8 (BASELINE config 5 as stated: e4m3 elements + one E8M0 scale per 32 K-elements) ---------------------------------
def mx_scales_rowmajor(scales: torch.Tensor, rows: int, K: int) -> torch.Tensor:
    """The quantiser's scale bytes (include/magma_hip.h: [chunk][block][row / 64][row % 16][(row % 64) / 16]) as a plain
    uint8 [rows, ceil(K / 128) * 4] matrix of E8M0 exponents, one per (row, 32-block)."""
    chunks, rg = (K + 127) // 128, (rows + 63) // 64
    v = scales.view(chunks, 4, rg, 16, 4).permute(2, 4, 3, 0, 1).reshape(rg * 64, chunks * 4)
    return v[:rows]


def mx_empty(M: int, N: int, device):
    """(q, scales) of an [M, N] MX operand for a GEMM epilogue to fill (``mx_out``): what quantize_mx_fp8 returns.  Columns
    N .. ceil(N / 128) * 128 of q are zeroed (the consumer's K loop reads whole 128-element chunks) and every scale byte is
    2^0 until written."""
    Kp = ceil_to(N, 128)
    q = torch.empty(M, Kp, dtype=torch.uint8, device=device)
    if Kp != N:
        q[:, N:].zero_()
    # scale bytes start at 127 (2^0), as the quantiser writes them for the zero blocks past N: the C8 epilogue only writes the
    # blocks with n < N, and the consuming GEMM walks whole 128-element chunks -- a leftover 0xFF byte is NaN in E8M0.  When every
    # byte WILL be written (whole 64-row groups, whole 128-column chunks: the training shapes) the fill launch is skipped.
    nbytes = int(L.load().mg_mx_scale_bytes(M, N))
    if M % 64 == 0 and Kp == N:
        return q, torch.empty(nbytes, dtype=torch.uint8, device=device)
    return q, torch.full((nbytes,), 127, dtype=torch.uint8, device=device)


def quantize_mx_fp8(x: torch.Tensor):
    """bf16 [M, K] -> (uint8 e4m3 [M, ldq] in K order, zero padded to ldq = ceil(K / 128) * 128; uint8 block scales in the
    layout of include/magma_hip.h mg_quantize_mx_fp8 -- mx_scales_rowmajor turns them into a [M, ldq / 32] matrix)."""
    _need_gpu(x)
    assert x.dtype == BF16 and x.ndim == 2 and x.stride(1) == 1
    M, K = x.shape
    ldq = ceil_to(K, 128)
    q = torch.empty(M, ldq, dtype=torch.uint8, device=x.device)
    nbytes = int(L.load().mg_mx_scale_bytes(M, K))
    if M % 64 == 0:      # whole 64-row groups: the kernel writes every scale byte (one per 32-column block of ldq, per row)
        scales = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    else:
        scales = torch.full((nbytes,), 127, dtype=torch.uint8, device=x.device)
    check(L.load().mg_quantize_mx_fp8(x.data_ptr(), x.stride(0), M, K, q.data_ptr(), ldq, scales.data_ptr(), _stream()),
          "mg_quantize_mx_fp8")
    return q, scales


def mx_dequant(q: torch.Tensor, scales: torch.Tensor, K: int) -> torch.Tensor:
    """fp32 [R, K] values an MX operand stands for (tests; the fp8 'dequantised oracle')."""
    R, ld = q.shape
    e = mx_scales_rowmajor(scales, R, ld).float()                                   # [R, ld / 32]
    v = q.view(torch.float8_e4m3fn).float().view(R, ld // 32, 32) * torch.exp2(e - 127.0)[:, :, None]
    return v.reshape(R, ld)[:, :K]


class PackedLinearMX:
    """A [N, K] weight as MX fp8: e4m3 bytes (row-major and / or fragment-tiled exactly like PackedLinearFP8 -- the tiling acts
    on the byte image) + E8M0 block scales [N, Kp / 128] int32."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, tiled: bool = True, rowmajor: bool = False):
        _need_gpu(weight)
        self.N, self.K = weight.shape
        assert self.K % 16 == 0, "fp8 GEMM needs K % 16 == 0"
        self.Kp = ceil_to(self.K, 128)
        n16 = ceil_to(self.N, 16)
        w = torch.zeros(n16, self.K, dtype=BF16, device=weight.device)
        w[: self.N] = weight.detach().to(BF16)
        q, sc = quantize_mx_fp8(w[: self.N])          # scale slabs are indexed by the weight's own row count
        if n16 != self.N:
            q = torch.cat([q, torch.zeros(n16 - self.N, q.shape[1], dtype=torch.uint8, device=q.device)])
        self.scales = sc
        self.bias = None if bias is None else bias.detach().to(torch.float32).contiguous()
        self.rm = q[: self.N].contiguous() if rowmajor else None
        self.ft = PackedLinear.tile(q.view(torch.int16)).view(torch.uint8) if tiled else None
        self._n16 = n16

    def dequant(self) -> torch.Tensor:
        q = self.rm if self.rm is not None else PackedLinear.untile(self.ft.view(torch.int16)).view(torch.uint8)[: self.N]
        return mx_dequant(q.contiguous(), self.scales, self.K)

    @classmethod
    def of_live(cls, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> "PackedLinearMX":
        """As PackedLinearFP8.of_live, with OCP MX block scales."""
        self = cls.__new__(cls)
        self.N, self.K = weight.shape
        assert weight.dtype == BF16 and weight.stride(1) == 1 and self.N % 16 == 0 and self.K % 128 == 0
        self.Kp, self._n16 = self.K, self.N
        q, self.scales = quantize_mx_fp8(weight)
        self.bias, self.rm = bias, None
        self.ft = PackedLinear.tile(q.view(torch.int16)).view(torch.uint8)
        return self


def gemm_mx_fp8(aq: torch.Tensor, a_scales: torch.Tensor, w: PackedLinearMX, out: Optional[torch.Tensor] = None, *,
                act: int = MG_ACT_NONE, residuals: Sequence[torch.Tensor] = (), act_after: int = MG_ACT_NONE, use_bias: bool = True,
                out_dtype=BF16, layout: Optional[str] = None, split_k: int = 0, act_n0: int = 0, tile: int = 0,
                aux=None, aux_mode: int = MG_AUX_NONE, aux_after: bool = False, out2: Optional[torch.Tensor] = None,
                mx_out=None, no_out: bool = False):
    """out[M,N] = epilogue(sum over 32-blocks of 2^(ea + ew) * (qa . qw)) on the block-scaled fp8 MFMA (fp32 accumulate).
    ``mx_out`` / ``no_out`` as for gemm_fp8."""
    _need_gpu(aq, a_scales)
    assert aq.dtype == torch.uint8 and aq.ndim == 2 and aq.stride(1) == 1 and aq.shape[1] == w.Kp
    M = aq.shape[0]
    assert a_scales.dtype == torch.uint8 and a_scales.numel() == int(L.load().mg_mx_scale_bytes(M, w.Kp))
    assert not no_out or (mx_out is not None and out is None)
    if out is None and not no_out:
        out = torch.empty(M, ceil_to(w.N, 8), dtype=out_dtype, device=aq.device)[:, : w.N]
    d = GemmDesc()
    d.A, d.lda = aq.data_ptr(), aq.stride(0)
    if layout is None:
        layout = "ft" if w.ft is not None else "rm"
    if layout == "ft":
        d.W, d.ldw, d.w_layout = w.ft.data_ptr(), w.Kp, MG_W_FRAGTILED
    else:
        d.W, d.ldw, d.w_layout = w.rm.data_ptr(), w.rm.stride(0), MG_W_ROWMAJOR
    d.M, d.N, d.K = M, w.N, w.Kp
    d.a_mode = MG_A_DENSE
    d.zero_page = zero_page(aq.device).data_ptr()
    d.tile_hint = tile
    d.split_k = split_k
    if split_k != 1:
        ws = splitk_workspace(aq.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    d.ep = _epilogue(out, w.N, w.bias if use_bias else None, None, act, residuals, act_after, aux, aux_mode, aux_after, out2,
                     mx_out=mx_out, M=M)
    d.ep.act_n0 = act_n0
    check(L.load().mg_gemm_mx_fp8(C.byref(d), a_scales.data_ptr(), w.scales.data_ptr(), _stream()), "mg_gemm_mx_fp8")
    return out


def debug_mx_mfma(a: torch.Tensor, sa: torch.Tensor, b: torch.Tensor, sb: torch.Tensor) -> torch.Tensor:
    """One v_mfma_scale_f32_16x16x128_f8f6f4 on explicit per-lane operands: a, b int32 [64, 8]; sa, sb int32 [64] -> fp32 [64, 4]."""
    _need_gpu(a, sa, b, sb)
    out = torch.empty(64, 4, dtype=torch.float32, device=a.device)
    check(L.load().mg_debug_mx_mfma(a.data_ptr(), sa.data_ptr(), b.data_ptr(), sb.data_ptr(), out.data_ptr(), _stream()), "mg_debug_mx_mfma")
    return out


def debug_mx_mfma_acc(form: int, a: torch.Tensor, sa: torch.Tensor, b: torch.Tensor, sb: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """One scaled f8f6f4 MFMA with its accumulator: form 16 = 16x16x128 (c and the result fp32 [64, 4]), form 32 = 32x32x64
    ([64, 16]); a, b int32 [64, 8]; sa, sb int32 [64] -> A B + c as the instruction forms it."""
    _need_gpu(a, sa, b, sb, c)
    n = {16: 4, 32: 16}[form]
    assert a.shape == (64, 8) and b.shape == (64, 8) and sa.shape == (64,) and sb.shape == (64,) and c.shape == (64, n)
    assert a.dtype == b.dtype == sa.dtype == sb.dtype == torch.int32 and c.dtype == torch.float32
    assert all(t.is_contiguous() for t in (a, sa, b, sb, c))
    out = torch.empty(64, n, dtype=torch.float32, device=a.device)
    check(L.load().mg_debug_mx_mfma_acc(form, a.data_ptr(), sa.data_ptr(), b.data_ptr(), sb.data_ptr(), c.data_ptr(), out.data_ptr(),
                                        _stream()), "mg_debug_mx_mfma_acc")
    return out
