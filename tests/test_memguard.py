"""tests/memguard.py on CPU tensors: planted stray writes around a guarded window are all seen, an untouched buffer passes, and a NaN left
in the interior is reported - for every element type the memory-contract tests use."""
import pytest
import torch

from memguard import GUARD_BYTES, GUARD_ROWS, PATTERN, damage, guarded, intact, poisoned, unwritten

TYPES = [torch.bfloat16, torch.float16, torch.float32]


def _base(big, view):
    return view.storage_offset() - big.storage_offset()


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("rows,cols,ld", [(5, 24, 40), (300, 200, 208), (3, 16, 16), (1, 8, 24)])
def test_layout_guards_and_alignment(dtype, rows, cols, ld):
    big, view = guarded((rows, cols), dtype, ld)
    es = big.element_size()
    g = _base(big, view)
    assert view.shape == (rows, cols) and (rows == 1 or view.stride(0) == ld) and view.stride(1) == 1
    assert view.data_ptr() % 16 == 0
    assert g >= GUARD_ROWS * ld and g * es >= GUARD_BYTES                       # the guard in front ...
    assert big.numel() - (g + rows * ld) == g                                  # ... and the same behind the last row's padding
    assert bool(torch.isnan(view.float()).all())                               # interior pre-filled with NaN
    assert bool((big.view(torch.uint8)[: g * es] == PATTERN).all())
    assert intact(big, view) and unwritten(view) == rows * cols


@pytest.mark.parametrize("dtype", TYPES)
def test_untouched_buffer_and_a_full_interior_write_pass(dtype):
    big, view = guarded((7, 24), dtype, 40)
    assert intact(big, view)
    view.copy_(torch.arange(7 * 24, dtype=torch.float32).reshape(7, 24))
    assert intact(big, view) and unwritten(view) == 0
    big2, view2 = guarded((7, 24), dtype, 24)                                   # ld == cols: no padding columns, guards only
    view2.zero_()
    assert intact(big2, view2) and unwritten(view2) == 0


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("where", ["before", "after", "middle_padding", "last_row_padding", "last_row_padding_end", "far_guard"])
def test_planted_write_is_seen(dtype, where):
    rows, cols, ld = 6, 24, 40
    big, view = guarded((rows, cols), dtype, ld)
    view.zero_()
    g = _base(big, view)
    at = {"before": g - 1,                                   # one element before the window
          "after": g + (rows - 1) * ld + cols,               # one element after the window's last element
          "middle_padding": g + 2 * ld + cols + 3,           # a padding column of a middle row
          "last_row_padding": g + (rows - 1) * ld + cols + 1,
          "last_row_padding_end": g + rows * ld - 1,
          "far_guard": big.numel() - 1}[where]
    assert intact(big, view)
    big[at] = 1.0
    assert not intact(big, view)
    assert str(at - g) in damage(big, view)
    assert unwritten(view) == 0                              # the interior itself is not what changed


def test_one_byte_of_a_guard_element_is_enough():
    big, view = guarded((4, 8), torch.float32, 12)
    view.zero_()
    raw = big.view(torch.uint8)
    raw[(_base(big, view) - 1) * 4 + 2] ^= 0x01
    assert not intact(big, view)


@pytest.mark.parametrize("dtype", TYPES)
def test_nan_left_in_the_interior_is_reported(dtype):
    big, view = guarded((5, 16), dtype, 24)
    view.zero_()
    assert unwritten(view) == 0
    view[3, 15] = float("nan")
    view[0, 0] = float("inf")
    assert unwritten(view) == 2 and intact(big, view)


def test_byte_filled_interior():
    big, view = guarded((5, 16), torch.bfloat16, 24, fill="bytes")
    assert bool((view.contiguous().view(torch.uint8) == PATTERN).all()) and unwritten(view) == 0


@pytest.mark.parametrize("dtype", TYPES)
def test_poisoned_input_keeps_its_values_between_nan(dtype):
    t = torch.arange(5 * 24, dtype=torch.float32).reshape(5, 24).to(dtype)
    p = poisoned(t, 40)
    assert torch.equal(p, t) and p.stride(0) == 40 and p.data_ptr() % 16 == 0
    flat = torch.as_strided(p, (5 * 40,), (1,))                                  # the window with its padding columns
    assert int(torch.isnan(flat.float()).sum()) == 5 * 16
    before = torch.as_strided(p, (64,), (1,), p.storage_offset() - 64)
    assert bool(torch.isnan(before.float()).all())
    img = torch.arange(2 * 3 * 4 * 8, dtype=torch.float32).reshape(2, 3, 4, 8).to(dtype)      # no leading dimension: guards only
    q = poisoned(img)
    assert q.shape == img.shape and q.is_contiguous() and torch.equal(q, img)
    behind = torch.as_strided(q, (64,), (1,), q.storage_offset() + img.numel())
    assert bool(torch.isnan(behind.float()).all())


def test_poisoned_integer_input_decodes_out_of_range():
    ids = torch.tensor([[0, 5, 48]], dtype=torch.int32)
    p = poisoned(ids)
    assert torch.equal(p, ids)
    around = torch.as_strided(p, (4,), (1,), p.storage_offset() - 4)
    assert bool((around < -(1 << 30)).all())
