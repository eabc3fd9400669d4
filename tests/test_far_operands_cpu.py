"""The far-operand case table (tests/far_operands.py) checked without a GPU: every view fits the arena, has rows on both sides of
the thresholds it claims, and every address a wrapped 32-bit offset could produce lies inside the arena and is not the true
one.  That last property is what makes the GPU tests safe to run: a kernel that wraps fails a comparison, it does not fault."""
import pytest
import torch

import far_operands as far


@pytest.fixture(scope="module")
def meta_arena():
    return torch.empty(far.ARENA_BYTES, dtype=torch.uint8, device="meta")


def test_sign_extension_by_hand():
    assert far.sext32(0) == 0 and far.sext32(2 ** 31 - 1) == 2 ** 31 - 1
    assert far.sext32(2 ** 31) == -2 ** 31 and far.sext32(2 ** 32 - 1) == -1
    assert far.sext32(2 ** 32 + 5) == 5 and far.sext32(-1) == -1


def test_aliases_by_hand():
    # a bf16 element at row 512 of a matrix with ld = 2^22 + 64: 2^31 + 2^15 elements, 2^32 + 2^16 bytes
    e = 512 * (2 ** 22 + 64)
    assert e == 2 ** 31 + 2 ** 15
    a = far.aliases(e, 2)
    assert a == {"byte_mod32": 2 ** 16, "byte_i32": 2 ** 16, "elem_i32": (-2 ** 31 + 2 ** 15) * 2, "elem_mod32": 2 * e,
                 "gemm_loader": 2 ** 16}
    assert set(far.wrapped(e, 2)) == {"byte_mod32", "byte_i32", "elem_i32", "gemm_loader"}
    # the element before the threshold: 2^32 - 2 bytes fit a uint32 but not an int; below 2^31 bytes nothing wraps
    assert far.wrapped(2 ** 31 - 1, 2) == {"byte_i32": -2}
    assert far.wrapped(2 ** 30 - 1, 2) == {}
    # fp32 at 2^30 elements = 2^32 bytes: only the byte forms wrap
    assert far.wrapped(2 ** 30, 4) == {"byte_mod32": 0, "byte_i32": 0, "gemm_loader": 2 ** 31}
    # bytes between 2^31 and 2^32 go negative as int, stay as uint32
    assert far.aliases(3 * 2 ** 30, 1)["byte_i32"] == -2 ** 30 and far.aliases(3 * 2 ** 30, 1)["byte_mod32"] == 3 * 2 ** 30
    # a uint32 element offset wraps at 2^32 elements only
    assert far.aliases(2 ** 32 + 7, 2)["elem_mod32"] == 14


def test_layout_by_hand():
    lay = far.far_layout(2, (600, 256), (2 ** 22 + 64, 1))
    assert lay.start == 2 ** 32 and lay.span == (599 * (2 ** 22 + 64) + 256) * 2
    assert lay.rows_past_elems31 == tuple(range(512, 600)) == lay.rows_past_bytes32
    lay = far.far_layout(4, (320, 264), (2 ** 22 + 64, 1))
    assert lay.start == 2 ** 33 and lay.rows_past_bytes32 == tuple(range(256, 320)) and lay.rows_past_elems31 == ()
    lay = far.far_layout(1, (600, 256), (2 ** 23 + 128, 1))
    assert lay.rows_past_elems31 == tuple(range(256, 600)) and lay.rows_past_bytes32 == tuple(range(512, 600))


def test_layout_refuses_what_ends_too_close_to_the_arena_end():
    with pytest.raises(ValueError, match="2\\^32 bytes before the end"):
        far.far_layout(4, (600, 264), (2 ** 22 + 64, 1))            # 10 GB behind an 8-GiB lead
    with pytest.raises(ValueError, match="2\\^32 bytes before the end"):
        far.far_layout(2, (600, 256), (2 ** 22 + 64, 1), arena_bytes=2 ** 33)
    with pytest.raises(ValueError, match="skew"):
        far.far_layout(2, (4, 8), (8, 1), skew=8)
    far.far_layout(4, (320, 264), (2 ** 22 + 64, 1))


@pytest.mark.parametrize("name", sorted(far.CASES))
def test_case_is_far_and_its_aliases_stay_inside(meta_arena, name):
    case = far.CASES[name]
    lay = case.layout()
    far.check_layout(lay, far.ARENA_BYTES, case.claims, elems_per_row=(0, 8, case.shape[-1] - 1))
    # the view the GPU test will use, on a meta arena: same offset, nothing out of range
    view, lay2 = far.far_view(meta_arena, case.dtype, lay.shape, lay.strides, case.skew)
    assert lay2 == lay and view.storage_offset() * lay.itemsize == lay.start and tuple(view.shape) == lay.shape
    last_byte = (view.storage_offset() + lay.last_offset() + 1) * lay.itemsize
    assert last_byte <= far.ARENA_BYTES - far.BYTES_32


def test_stray_write_check_finds_one_byte():
    """poison / wipe / assert_arena_poison on a small CPU arena: a view's own writes are wiped, one byte anywhere else is found."""
    arena = torch.zeros(1 << 16, dtype=torch.uint8)
    far.poison(arena)
    far.assert_arena_poison(arena, "fresh")
    assert bool(torch.isnan(arena.view(torch.bfloat16)).all()) and bool(torch.isnan(arena.view(torch.float32)).all())
    for dtype in (torch.bfloat16, torch.float32, torch.uint8):
        view = arena.view(dtype).as_strided((5, 24), (100, 1), 64)
        view.fill_(1)
        with pytest.raises(AssertionError, match="written outside the operand"):
            far.assert_arena_poison(arena, "view written")
        far.wipe(view)
        far.assert_arena_poison(arena, "view wiped")
    arena[40001] = 0xFE
    with pytest.raises(AssertionError, match="first at byte 40000"):
        far.assert_arena_poison(arena, "one stray byte")


def test_gemm256_refusal_stride_is_the_first_one_past_the_limit():
    """256 rows at the limit stride span exactly 2^32 bytes: the per-lane byte offset of the 256x256 loaders (at most 255 rows
    and one row's K-tile) no longer fits a uint32 for every ld at or past it, and does below it."""
    ld = far.GEMM256_LD_LIMIT
    assert 256 * ld * 2 == far.BYTES_32
    assert 255 * (ld - 8) * 2 + 64 * 2 < far.BYTES_32
    assert far.LD22 < ld and far.LD23B // 2 < ld          # the far cases themselves stay on the 256x256 kernel
