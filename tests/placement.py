"""Operands at non-minimal leading dimensions and misaligned addresses, inside a parent buffer
whose every other element is known.

`placed(t, ld, off, fill)` copies `t` into a fresh 1-D parent and returns the strided view of
the parent that holds `t`'s values: it starts `off` elements into the parent, its rows are `ld`
elements apart (N-D: `strides=` gives every stride), and the parent ends TAIL elements after
the view's last element.  Everything that is not the view (the head, the gaps between rows,
the tail) holds `fill`, a 32-bit pattern:

    NAN       a quiet NaN: for inputs, so a read of any gap element shows in the result;
    SENTINEL  a NaN with a payload no arithmetic produces: for outputs;
    ZERO      zeros (the CPU reference's own placement check).

`check_gaps(view)` asserts that every non-view element of the parent still holds the fill bit
for bit, and otherwise names the first and last changed parent offsets and where they lie
relative to the view's rows.  `out(shape, ld, off)` is an output placement: a NaN payload (an
element the kernel never stores stays NaN) between SENTINEL gaps.

With device="cuda" the parent goes through guard.put: inside a guard.allocations context it
lives in a poisoned, band-checked arena at a 512-byte-aligned address, outside one at a fresh
caching-allocator block, so `view.data_ptr() % 16 == 4 * off % 16` either way and accesses past
the parent land in a checked band."""
import torch

import guard

NAN = 0x7FC00000
SENTINEL = 0x7FC5A3E1
ZERO = 0
TAIL = 5  # parent elements after the view's last one

_INT_OF = {4: torch.int32, 8: torch.int64, 2: torch.int16}


def _extent(shape, strides):
    return 1 + sum((n - 1) * s for n, s in zip(shape, strides))


def row_strides(shape, ld):
    """Strides of a view of `shape` whose rows (the last dim) are `ld` elements apart and
    whose outer dims are packed over those rows (a (B, R, ld) buffer read as (B, R, C))."""
    strides = [1] * len(shape)
    if len(shape) >= 2:
        strides[-2] = ld
        for d in range(len(shape) - 3, -1, -1):
            strides[d] = strides[d + 1] * shape[d + 1]
    return tuple(strides)


def placed(t, ld=None, off=0, fill=NAN, strides=None, device=None):
    """The view described in the module docstring.  `t` is a host tensor of a 2-, 4- or 8-byte
    dtype; `ld` defaults to the dense row length; `device` None keeps the parent on the host."""
    t = t.detach().cpu()
    shape = tuple(t.shape)
    assert all(n > 0 for n in shape) and off >= 0
    if strides is None:
        strides = row_strides(shape, shape[-1] if ld is None else ld)
    strides = tuple(int(s) for s in strides)
    assert len(strides) == len(shape) and strides[-1] == 1
    if len(shape) >= 2:
        assert strides[-2] >= shape[-1], "rows overlap"
    idx = torch.arange(off + _extent(shape, strides)).as_strided(shape, strides, off)
    assert idx.unique().numel() == idx.numel(), "the view overlaps itself"
    n = off + _extent(shape, strides) + TAIL
    bits = _INT_OF[t.element_size()]
    host = torch.empty(n, dtype=bits).fill_(_signed(fill, bits)).view(t.dtype)
    host.as_strided(shape, strides, off).copy_(t)
    parent = guard.put(host, device) if device is not None else host
    view = parent.as_strided(shape, strides, parent.storage_offset() + off)  # (an arena's lead)
    gap = torch.ones(n, dtype=torch.bool)
    gap[idx.flatten()] = False
    view._placement = (parent, gap, fill, off, strides)
    return view


def out(shape, ld=None, off=0, device=None, strides=None):
    """An output placement: NaN payload, SENTINEL gaps."""
    return placed(torch.full(tuple(shape), float("nan")), ld, off, SENTINEL, strides, device)


def _signed(pattern, bits):
    width = 8 * torch.empty(0, dtype=bits).element_size()
    pattern &= (1 << width) - 1
    return pattern - (1 << width) if pattern >> (width - 1) else pattern


def parent_of(view):
    return view._placement[0]


def gap_count(view):
    return int(view._placement[1].sum())


def check_gaps(view, what="output"):
    """Every parent element outside `view` holds its fill bit for bit."""
    parent, gap, fill, off, strides = view._placement
    bits = _INT_OF[parent.element_size()]
    now = parent.detach().cpu().view(bits)
    bad = ((now != _signed(fill, bits)) & gap).nonzero().flatten()
    if bad.numel() == 0:
        return
    first, last = int(bad[0]), int(bad[-1])

    def where(p):
        if p < off:
            return f"{off - p} element(s) before the view"
        if len(strides) < 2:
            return f"{p - off - (view.shape[-1] - 1)} element(s) past the view's end"
        row, col = divmod(p - off, strides[-2])
        return (f"row {row} column {col} of the view's rows of stride {strides[-2]} "
                f"(the payload ends at column {view.shape[-1] - 1})")
    raise AssertionError(
        f"{what}: {bad.numel()} gap element(s) of the parent were written (fill 0x{fill:08X}): "
        f"parent offsets {first} .. {last}; first is {where(first)}, last is {where(last)}; "
        f"view shape {tuple(view.shape)} strides {strides} offset {off}")
