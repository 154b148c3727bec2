"""Guard / stride / poison helpers for the memory-contract tests (plain torch: the same code runs on a CPU tensor and on the GPU).

A kernel's arithmetic is checked against references elsewhere; these helpers pin WHERE it reads and writes:

  guarded(shape, dtype, ld)   an output window [rows, cols] with row stride ld >= cols inside ONE allocation, a guard band on either
                              side.  Guards and padding columns hold the byte PATTERN, the interior NaN (or the pattern as well).
  intact(big, view)           every byte outside the window's [rows, cols] still holds the pattern.
  unwritten(view)             how many interior elements the kernel left non-finite (the NaN pre-fill: "every element is written").
  poisoned(t, ld)             an input copied into such a window whose padding columns and guards are NaN (integers: the pattern,
                              which decodes to a large negative number): a kernel that looks where its contract says it does not, sees it.

The bands are compared as BYTES, so the check is exact for bf16 / fp16 / fp32 alike (a float marker would have to be representable in
every type).  A guard is at least 256 rows of the window's leading dimension and at least 1 MiB: an overreach of one whole row tile
lands in memory the test owns - and is seen there - instead of in a neighbouring allocation.  Nothing here is meant to fault.
Window bases stay 16-byte aligned (the guard is a multiple of 16 elements behind torch's own allocation alignment); a caller keeps ld a
multiple of 8 (16-bit types) / 4 (fp32), as the launchers ask."""
import torch

PATTERN = 0xA5                   # bf16 / fp16 0xA5A5 = a negative denormal-sized number, fp32 0xA5A5A5A5 = -2.87e-16, int32 = -1515870811
GUARD_ROWS = 256
GUARD_BYTES = 1 << 20


def _guard_elems(ld, itemsize):
    n = max(GUARD_ROWS * ld, -(-GUARD_BYTES // itemsize))
    return -(-n // 16) * 16


def guarded(shape, dtype, ld=None, fill="nan", device="cpu"):
    """(big, view): `view` = the [rows, cols] window (row stride ld) of the flat allocation `big`.  fill: "nan" pre-fills the interior
    with NaN (floating types), "bytes" leaves the pattern there too."""
    rows, cols = shape
    ld = cols if ld is None else ld
    assert rows >= 1 and cols >= 1 and ld >= cols, (shape, ld)
    itemsize = torch.empty(0, dtype=dtype).element_size()
    g = _guard_elems(ld, itemsize)
    big = torch.full(((2 * g + rows * ld) * itemsize,), PATTERN, dtype=torch.uint8, device=device).view(dtype)
    view = big[g:g + rows * ld].view(rows, ld)[:, :cols]
    assert view.data_ptr() % 16 == 0
    if fill == "nan":
        assert dtype.is_floating_point, "NaN pre-fill needs a floating type"
        view.fill_(float("nan"))
    else:
        assert fill == "bytes", fill
    return big, view


def _outside(big, view):
    """uint8 copy of `big` with the window's own bytes overwritten by the pattern: what must still be all-pattern."""
    assert view.dim() == 2 and view.stride(1) == 1 and view.untyped_storage().data_ptr() == big.untyped_storage().data_ptr()
    rows, cols = view.shape
    ld = view.stride(0) if rows > 1 else None
    es = big.element_size()
    off = view.storage_offset() - big.storage_offset()
    if ld is None:                                        # a one-row window has no stride of its own: it ends at its last column
        ld = cols
    b = big.view(torch.uint8).clone()
    last = off + (rows - 1) * ld + cols                   # one past the window's last element
    assert off >= 0 and last <= big.numel()
    full = b[off * es:(off + (rows - 1) * ld) * es].view(rows - 1, ld * es)
    full[:, :cols * es] = PATTERN
    b[(off + (rows - 1) * ld) * es:last * es] = PATTERN
    return b


def intact(big, view):
    """True when every byte of `big` outside view's [rows, cols] is unchanged: both guards and the padding columns of every row."""
    return bool((_outside(big, view) == PATTERN).all())


def damage(big, view):
    """For a failing intact(): the element offsets (relative to the window's first element) of the first few changed bytes."""
    es = big.element_size()
    bad = torch.nonzero(_outside(big, view) != PATTERN).flatten()
    off = view.storage_offset() - big.storage_offset()
    return f"{bad.numel()} bytes changed outside the window; element offsets from the window base: {sorted({int(i) // es - off for i in bad[:8].tolist()})}"


def unwritten(view):
    """Number of non-finite elements inside the window: after a NaN pre-fill, the elements the kernel never wrote (or wrote NaN to)."""
    return int((~torch.isfinite(view.float())).sum())


def poisoned(t, ld=None):
    """A copy of input `t` whose surroundings are poison.  2-D t: a [rows, cols] window with row stride ld (>= cols, default cols) whose
    padding columns and guards are NaN.  Any other rank: the contiguous tensor between two NaN guards (operands without a leading
    dimension, such as an NHWC image or a bias vector), in t's shape; its "row" for the guard size is its last dimension (one element
    for a vector).  Integer types get the byte pattern (a large negative value) instead of NaN."""
    shape = t.shape
    t2 = t if t.dim() == 2 else t.reshape(-1, shape[-1] if t.dim() > 2 else 1)
    rows, cols = t2.shape
    big, view = guarded((rows, cols), t.dtype, ld if t.dim() == 2 else None, fill="bytes", device=t.device)
    if t.dtype.is_floating_point:
        big.fill_(float("nan"))
    view.copy_(t2)
    return view if t.dim() == 2 else view.reshape(shape)
