"""Operands past 4 GiB: one arena, far views, alias arithmetic and the case table of the far-operand tests.

The contract under test (include/magma_hip.h): an operand of any size is either addressed correctly or refused with an error,
never misread.  A kernel that keeps an offset in 32 bits breaks it silently once an operand spans 2^32 bytes or 2^31 elements:
it reads (or writes) another place of the same buffer.  The tests therefore put ONE operand of each op into a 17-GiB arena so
that

  * the operand's first element lies at least 2^31 elements (of its type) behind the arena's start, and its last byte at least
    2^32 bytes before the arena's end: every address a wrapped offset can produce -- see ``aliases`` -- lies INSIDE the arena;
  * the arena is 0xFF everywhere else (NaN as bf16 and fp32, 255 as uint8): a wrapped read returns poison or another row and
    fails the comparison with the reference, a wrapped store is found by ``assert_arena_poison``.  Neither leaves the allocation.

Everything here is integer arithmetic and torch views: importing the module needs no GPU (test_far_operands_cpu.py checks the
case table on "meta" tensors; test_far_operands_gpu.py runs the same table)."""
from dataclasses import dataclass, field
from typing import Tuple

import torch

ARENA_BYTES = 2 ** 34 + 2 ** 30          # 17 GiB
BYTES_32 = 2 ** 32                       # first byte offset a uint32 cannot hold
ELEMS_31 = 2 ** 31                       # first element offset an int cannot hold
POISON = 0xFF
CHUNK = 2 ** 30                          # the arena is compared in pieces of at most 1 GiB
MIN_ROWS_PAST = 8

ITEMSIZE = {torch.uint8: 1, torch.bfloat16: 2, torch.float32: 4, torch.int64: 8}
SAME_SIZE_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


# ---------------------------------------------------------------------------------------------------------------------------
# alias arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def sext32(x: int) -> int:
    """The low 32 bits of x as a signed integer (what a cast to ``int`` keeps)."""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


def aliases(elem_off: int, itemsize: int) -> dict:
    """BYTE offsets (from the operand's base pointer) that a kernel with a 32-bit offset somewhere could touch instead of the
    element at ``elem_off``; the true one is ``elem_off * itemsize``.  An entry equal to the true offset means that form does
    not wrap for this element."""
    t = elem_off * itemsize
    return {
        "byte_mod32": t % BYTES_32,                               # uint32_t byte offset
        "byte_i32": sext32(t),                                    # int byte offset, sign-extended
        "elem_i32": sext32(elem_off) * itemsize,                  # int element offset, sign-extended, scaled in 64 bits
        "elem_mod32": (elem_off % BYTES_32) * itemsize,           # uint32_t element offset, scaled in 64 bits
        "gemm_loader": ((sext32(elem_off) & 0xFFFFFFFF) * 2) % BYTES_32,   # (uint32_t)(int)e * 2u of the 256x256 GEMM's loaders
    }


def wrapped(elem_off: int, itemsize: int) -> dict:
    """The aliases that differ from the truth."""
    t = elem_off * itemsize
    return {k: v for k, v in aliases(elem_off, itemsize).items() if v != t}


# forms that must wrap once an element is past a threshold (the others may: a uint32 element offset only wraps at 2^32 elements,
# which no case reaches)
WRAPS_PAST = {"bytes32": ("byte_mod32", "byte_i32"), "elems31": ("elem_i32",)}


# ---------------------------------------------------------------------------------------------------------------------------
# placement
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class FarLayout:
    """Where a strided view lies in the arena (bytes from the arena's start) and which of its rows are far.  A "row" is an index
    of dimension 0; its offset is that of its first element, counted from the view's base pointer as a kernel counts it."""
    itemsize: int
    shape: Tuple[int, ...]
    strides: Tuple[int, ...]          # elements
    start: int                        # byte offset of element 0 in the arena
    span: int                         # bytes from element 0 to the end of the last element
    rows_past_bytes32: Tuple[int, ...]
    rows_past_elems31: Tuple[int, ...]

    def row_offset(self, r: int) -> int:
        return r * self.strides[0]

    def last_offset(self) -> int:
        return sum((n - 1) * s for n, s in zip(self.shape, self.strides))

    def rows_below(self, what: str) -> Tuple[int, ...]:
        past = set(self.rows_past_bytes32 if what == "bytes32" else self.rows_past_elems31)
        return tuple(r for r in range(self.shape[0]) if r not in past)


def far_layout(itemsize: int, shape, strides, arena_bytes: int = ARENA_BYTES, skew: int = 0) -> FarLayout:
    """Place a view: element 0 at 2^31 elements (+ ``skew`` bytes, a multiple of 16) behind the arena's start.  Refuses a view
    whose end is less than 2^32 bytes before the arena's end, and one with a negative or overlapping-by-design stride of 0."""
    shape, strides = tuple(int(n) for n in shape), tuple(int(s) for s in strides)
    if len(shape) != len(strides) or not shape or any(n <= 0 for n in shape) or any(s <= 0 for s in strides):
        raise ValueError(f"far_layout: bad shape / strides {shape} / {strides}")
    if skew < 0 or skew % 16:
        raise ValueError("far_layout: skew must be a non-negative multiple of 16 bytes")
    start = ELEMS_31 * itemsize + skew
    last = sum((n - 1) * s for n, s in zip(shape, strides))
    span = (last + 1) * itemsize
    if start + span > arena_bytes - BYTES_32:
        raise ValueError(f"far_layout: a view of {span} bytes at {start} ends less than 2^32 bytes before the end of an arena of "
                         f"{arena_bytes} bytes")
    rows = range(shape[0])
    return FarLayout(itemsize, shape, strides, start, span,
                     tuple(r for r in rows if r * strides[0] * itemsize >= BYTES_32),
                     tuple(r for r in rows if r * strides[0] >= ELEMS_31))


def far_view(arena: torch.Tensor, dtype, shape, strides, skew: int = 0):
    """(view, FarLayout): a strided view of ``arena`` (1-D uint8, any device -- "meta" included) placed by far_layout."""
    assert arena.dtype == torch.uint8 and arena.ndim == 1
    lay = far_layout(ITEMSIZE[dtype], shape, strides, arena.numel(), skew)
    typed = arena.view(dtype)
    return typed.as_strided(lay.shape, lay.strides, lay.start // lay.itemsize), lay


def check_layout(lay: FarLayout, arena_bytes: int, claims, elems_per_row=(0,)) -> None:
    """What test_far_operands_cpu.py asserts of every case: the view fits, it has rows on both sides of each threshold it
    claims, and every alias of the checked elements (first and last element of every far row, plus ``elems_per_row``) lies inside
    the arena and, for the forms that must wrap past a claimed threshold, differs from the true address."""
    assert lay.start >= ELEMS_31 * lay.itemsize and lay.start % 16 == 0
    assert lay.start + lay.span <= arena_bytes - BYTES_32
    row_last = lay.last_offset() - (lay.shape[0] - 1) * lay.strides[0]       # last element of a row, from the row's start
    for what in claims:
        past = lay.rows_past_bytes32 if what == "bytes32" else lay.rows_past_elems31
        assert len(past) >= MIN_ROWS_PAST, f"{what}: only {len(past)} rows past the threshold"
        assert len(lay.rows_below(what)) >= 1, f"{what}: no row below the threshold"
        for r in past:
            for e in {0, row_last, *elems_per_row}:
                off = lay.row_offset(r) + e
                t = off * lay.itemsize
                al = aliases(off, lay.itemsize)
                for form, a in al.items():
                    addr = lay.start + a
                    assert 0 <= addr and addr + 16 <= arena_bytes, f"alias {form} of row {r} leaves the arena: {addr}"
                for form in WRAPS_PAST[what]:
                    assert al[form] != t, f"row {r} is past {what} but its {form} alias is the true address"
                if lay.itemsize == 2 and what == "elems31":
                    assert al["gemm_loader"] != t


# ---------------------------------------------------------------------------------------------------------------------------
# poison and the stray-write check (GPU side; plain torch)
# ---------------------------------------------------------------------------------------------------------------------------
def poison(arena: torch.Tensor) -> None:
    arena.fill_(POISON)


def as_ints(view: torch.Tensor) -> torch.Tensor:
    """The same memory as integers of the element size (strided views keep their strides)."""
    return view.view(SAME_SIZE_INT[view.element_size()])


def wipe(*views: torch.Tensor) -> None:
    """Back to 0xFF: the regions an op may legitimately have written."""
    for v in views:
        ints = as_ints(v)
        ints.fill_(POISON if ints.dtype == torch.uint8 else -1)


def assert_arena_poison(arena: torch.Tensor, what: str = "") -> None:
    """Every byte of the arena is 0xFF, compared as int64 against -1 in pieces of at most 1 GiB (no temporary of arena size)."""
    words = arena.view(torch.int64)
    step = CHUNK // 8
    for i in range(0, words.numel(), step):
        piece = words[i:i + step]
        if not bool((piece == -1).all()):
            first = int((piece != -1).nonzero()[0]) + i
            raise AssertionError(f"{what}: the arena was written outside the operand: first at byte {first * 8} "
                                 f"(word {hex(int(piece[first - i]) & (2 ** 64 - 1))})")


# ---------------------------------------------------------------------------------------------------------------------------
# the case table (shared by the CPU and GPU tests)
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class FarCase:
    op: str                           # the op and which of its operands is far
    dtype: torch.dtype
    shape: Tuple[int, ...]
    strides: Tuple[int, ...]
    claims: Tuple[str, ...] = ("bytes32", "elems31")
    pad_cols: int = 0                 # columns behind the view's own that the op may write too (documented padding)
    skew: int = 0                     # bytes behind the usual place (a second operand of the same op in the arena)
    extra: dict = field(default_factory=dict, compare=False, hash=False)

    def layout(self, arena_bytes: int = ARENA_BYTES) -> FarLayout:
        shape = self.shape[:-1] + (self.shape[-1] + self.pad_cols,)
        return far_layout(ITEMSIZE[self.dtype], shape, self.strides, arena_bytes, self.skew)


BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
LD22 = 2 ** 22 + 64                   # bf16 / fp32 rows: row 512 starts past 2^31 elements; fp32 row 256 past 2^32 bytes
LD23B = 2 ** 23 + 128                 # uint8 rows: row 256 starts past 2^31 elements, row 512 past 2^32 bytes
LD28 = 2 ** 28 + 8                    # 16 rows: row 8 starts past 2^31 elements
GEMM_M, GEMM_K, GEMM_N = 600, 256, 264
# fp32 rows of LD22 elements behind their 8-GiB lead: 320 rows end 4 GiB before the arena's end; rows from 256 on are past 2^32
# bytes, none reaches 2^31 elements (that threshold is covered by the bf16 cases)
F32_ROWS = 320

CASES = {
    # --- tile GEMMs (mg_gemm_bf16): tile 128 / 256, split_k 1 / 2, row-major / fragment-tiled W where that applies
    "gemm_a": FarCase("gemm: A", BF16, (GEMM_M, GEMM_K), (LD22, 1)),
    "gemm_w": FarCase("gemm: row-major W", BF16, (GEMM_M, GEMM_K), (LD22, 1)),
    "gemm_out_bf16": FarCase("gemm: bf16 output", BF16, (GEMM_M, GEMM_N), (LD22, 1)),
    "gemm_out_f32": FarCase("gemm: fp32 output", F32, (F32_ROWS, GEMM_N), (LD22, 1), claims=("bytes32",)),
    "gemm_residual": FarCase("gemm: residual", BF16, (GEMM_M, GEMM_N), (LD22, 1)),
    "gemm_aux": FarCase("gemm: aux", BF16, (GEMM_M, GEMM_N), (LD22, 1)),
    "gemm_out2": FarCase("gemm: out2", BF16, (GEMM_M, GEMM_N), (LD22, 1)),
    # --- quantised A of the fp8 GEMMs: uint8 rows
    "gemm_fp8_a": FarCase("gemm_fp8 / gemm_mx_fp8: A", U8, (GEMM_M, GEMM_K), (LD23B, 1)),
    # --- skinny GEMV
    "skinny_x": FarCase("gemm_skinny: x", BF16, (16, 1024), (LD28, 1)),
    "skinny_out": FarCase("gemm_skinny: output", BF16, (16, GEMM_N), (LD28, 1)),
    # --- row and movement kernels
    "layernorm_x": FarCase("layernorm: x", BF16, (GEMM_M, 264), (LD22, 1)),
    "layernorm_out": FarCase("layernorm: out", BF16, (GEMM_M, 264), (LD22, 1)),
    "layernorm_bwd_x": FarCase("layernorm_bwd: x", BF16, (GEMM_M, 264), (LD22, 1)),
    "layernorm_bwd_dy": FarCase("layernorm_bwd: dy", BF16, (GEMM_M, 264), (LD22, 1)),
    "ce_logits": FarCase("cross_entropy / cross_entropy_fwd_bwd / argmax / token_logprobs: fp32 logits", F32, (F32_ROWS, 1053), (LD22, 1),
                         claims=("bytes32",)),
    "colsum_x": FarCase("colsum (atomic and deterministic): x", BF16, (GEMM_M, 264), (LD22, 1)),
    "transpose_in": FarCase("transpose / transpose_colsum: input", BF16, (GEMM_M, 72), (LD22, 1)),
    "transpose_out": FarCase("transpose: output [C, round_up(R, 8)] of an input [37, 600]", BF16, (GEMM_M, 37), (LD22, 1), pad_cols=3),
    "gelu_x": FarCase("gelu_erf: x", BF16, (GEMM_M, 264), (LD22, 1)),
    "gelu_out": FarCase("gelu_erf: out", BF16, (GEMM_M, 264), (LD22, 1)),
    "scale_rows_src": FarCase("scale_rows_acc: fp32 src", F32, (F32_ROWS, 264), (LD22, 1), claims=("bytes32",)),
    "quantize_rows_x": FarCase("quantize_rows_fp8: x", BF16, (GEMM_M, 256), (LD22, 1)),
    "quantize_mx_x": FarCase("quantize_mx_fp8: x", BF16, (GEMM_M, 256), (LD22, 1)),
    "head_transpose_src": FarCase("head_transpose: src [1, 600, 1, 256] at a far ss", BF16, (GEMM_M, 256), (LD22, 1)),
    "rotary_qkv": FarCase("rotary_split: fused qkv rows [600, 3 * 256] at a far ld_qkv", BF16, (GEMM_M, 768), (LD22, 1)),
    "embedding_out": FarCase("embedding: out [16, 4, 64] at a far out_bstride", BF16, (16, 4, 64), (LD28, 64, 1)),
}

# contiguous KV caches [130, 16, 4096, 256] bf16, 4.36 GB each, K and V behind one another; their rows here are (batch, head)
# pairs: batch row 128 starts at exactly 2^31 elements = 2^32 bytes
KV_B, KV_H, KV_SMAX = 130, 16, 4096
KV_BYTES = KV_B * KV_H * KV_SMAX * 256 * 2
CASES["kv_cache_k"] = FarCase("decode attention / cache append: K cache", BF16, (KV_B * KV_H, KV_SMAX, 256), (KV_SMAX * 256, 256, 1))
CASES["kv_cache_v"] = FarCase("decode attention / cache append: V cache", BF16, (KV_B * KV_H, KV_SMAX, 256), (KV_SMAX * 256, 256, 1),
                              skew=KV_BYTES)

# kv_reorder's two staging caches: views of the same rows KV_STAGE_SHIFT positions further on.  The op touches only the first
# d_pos positions of a row (at most 80 here), so staging position i lies on the unused position KV_STAGE_SHIFT + i of K / V.
KV_STAGE_SHIFT = 1024
CASES["kv_stage_k"] = FarCase("kv_reorder: K staging cache", BF16, (KV_B * KV_H, KV_SMAX, 256), (KV_SMAX * 256, 256, 1),
                              skew=KV_STAGE_SHIFT * 512)
CASES["kv_stage_v"] = FarCase("kv_reorder: V staging cache", BF16, (KV_B * KV_H, KV_SMAX, 256), (KV_SMAX * 256, 256, 1),
                              skew=KV_BYTES + KV_STAGE_SHIFT * 512)

# the MX output copy of the fp8 GEMMs is dense by contract (ldc8 == ceil(N / 128) * 128): a far one is a real 4.33-GB output
CASES["gemm_mx_out"] = FarCase("gemm_fp8: dense MX output copy [66048, 65536]", U8, (65536 + 512, 65536), (65536, 1))

# refusals of the 256x256 GEMM's dispatcher: 256 rows of A (or of a row-major W) must span less than 2^32 bytes
GEMM256_LD_LIMIT = 2 ** 23            # elements of 2 bytes
