"""Guard-banded, poisoned allocation for kernel tests.

`with guard.allocations(fill) as g:` replaces, for the duration of the block, the torch
factories the product allocates through (torch.empty / empty_like / zeros / zeros_like / full /
full_like / ones / ones_like and Tensor.new_empty / new_zeros / new_full / new_ones).  Every
device tensor they create then lives in an arena of its own:

    [ leading band >= 64 KiB | payload: exactly the bytes the tensor spans | trailing band 64 KiB ]

The payload starts at a 512-byte-aligned address (as caching-allocator blocks do, so every
alignment-dependent dispatch takes the path it takes in the product) and the trailing band
starts at the very next byte after it.  Shape, dtype and strides are the ones the original
factory gives for the same call (asked of it on device="meta").

Poison.  Bands, and the payload of empty / empty_like / new_empty, hold the context's fill byte:
FILL_A = 0xFF (NaN as fp32 / bf16 / fp16 / fp64, -1 as a uint8-workspace counter) or
FILL_B = 0x7F (about 3.4e38 as fp32 / bf16, finite as fp64).  A max or min can swallow a NaN and
a multiply by zero a finite value; the two fills together catch both.  Float dtypes and uint8
(the product's workspaces) get the poison; integer and bool dtypes get zero bands and a zero
prefill under both fills, so a stray read of an index can never point outside its table.

The context keeps every arena alive until `g.check()`, which asserts that every band still
holds its fill byte for byte and otherwise names the tensor (shape, dtype, allocating file:line),
the side and the first and last dirty offsets.  `guard.put(t)` copies a host or device tensor
into a guarded one (test inputs, `p.data = guard.put(p.data)` for parameters); outside a context
it is a plain copy to the device, so one test body serves guarded and unguarded runs.
`guard.owns(t)` says whether a tensor lives in an arena of the active (or last) context.

Only calls for `device_type` ("cuda" unless the harness itself is under test on "cpu") are
intercepted; all others pass through untouched.  The patching lives only inside the `with`
block and is undone in a `finally`; the context refuses to start or allocate while a stream is
capturing."""
import contextlib
import os
import sys
import threading

import torch

BAND = 64 * 1024
ALIGN = 512
FILL_A = 0xFF
FILL_B = 0x7F

_HERE = os.path.abspath(__file__)
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__))
PRODUCT = os.sep + "e2ep_amd" + os.sep  # a path with this in it is the product's runtime package

# name -> (prefill kind, takes its spec from a tensor in args[0])
_FACTORIES = {
    "empty": ("poison", False), "empty_like": ("poison", True),
    "zeros": ("zero", False), "zeros_like": ("zero", True),
    "ones": ("one", False), "ones_like": ("one", True),
    "full": ("value", False), "full_like": ("value", True),
}
_METHODS = {"new_empty": "poison", "new_zeros": "zero", "new_ones": "one", "new_full": "value"}

_active = None  # the context whose `with` block is running
_last = None    # the most recent context (owns() after the block)


class GuardError(AssertionError):
    pass


def _poisoned(dtype):
    return dtype.is_floating_point or dtype.is_complex or dtype == torch.uint8


def _span_bytes(size, stride, itemsize):
    if any(s == 0 for s in size):
        return 0
    return (1 + sum((n - 1) * st for n, st in zip(size, stride))) * itemsize


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _site():
    """file:line of the allocating call: the innermost frame in e2ep_amd/, else the innermost
    frame outside this module and torch."""
    f = sys._getframe(1)
    first = None
    while f is not None:
        fn = os.path.abspath(f.f_code.co_filename)
        if fn != _HERE and not fn.startswith(_TORCH_DIR):
            here = f"{fn}:{f.f_lineno}"
            if PRODUCT in fn:
                return here
            first = first or here
        f = f.f_back
    return first or "?"


class Arena:
    __slots__ = ("raw", "lead", "nbytes", "byte", "shape", "dtype", "site", "kind")

    def __init__(self, raw, lead, nbytes, byte, shape, dtype, site, kind):
        self.raw, self.lead, self.nbytes, self.byte = raw, lead, nbytes, byte
        self.shape, self.dtype, self.site, self.kind = shape, dtype, site, kind

    def bands(self):
        return (("leading", self.raw[:self.lead]), ("trailing", self.raw[self.lead + self.nbytes:]))

    def describe(self):
        return f"{self.kind} {tuple(self.shape)} {self.dtype} allocated at {self.site}"


class allocations(contextlib.AbstractContextManager):
    def __init__(self, fill, device_type="cuda"):
        assert fill in (FILL_A, FILL_B), "fill is guard.FILL_A (0xFF) or guard.FILL_B (0x7F)"
        self.fill = fill
        self.device_type = device_type
        self.arenas = []
        self.bytes = 0
        self._storages = {}
        self._orig = {}
        self._orig_methods = {}
        self._tls = threading.local()
        self._lock = threading.Lock()

    # -- patching ---------------------------------------------------------------------------
    def __enter__(self):
        global _active, _last
        if _active is not None:
            raise GuardError("guard.allocations does not nest")
        if _capturing():
            raise GuardError("guard.allocations refuses to start while a stream is capturing")
        try:
            for name, (kind, like) in _FACTORIES.items():
                self._orig[name] = getattr(torch, name)
                setattr(torch, name, self._wrap(name, self._orig[name], kind, like, False))
            for name, kind in _METHODS.items():
                self._orig_methods[name] = getattr(torch.Tensor, name)
                setattr(torch.Tensor, name, self._wrap(name, self._orig_methods[name], kind, True, True))
        except BaseException:
            self._restore()
            raise
        _active = _last = self
        return self

    def __exit__(self, *exc):
        global _active
        try:
            self._restore()
        finally:
            _active = None
        return False

    def _restore(self):
        for name, fn in self._orig.items():
            setattr(torch, name, fn)
        for name, fn in self._orig_methods.items():
            setattr(torch.Tensor, name, fn)
        self._orig, self._orig_methods = {}, {}

    def _wrap(self, name, orig, kind, like, method):
        def factory(*args, **kwargs):
            # re-entrancy: torch's meta implementation of full() calls torch.empty itself
            if getattr(self._tls, "busy", False) or kwargs.get("out") is not None:
                return orig(*args, **kwargs)
            device = kwargs.get("device")
            if device is None and like and args and isinstance(args[0], torch.Tensor):
                device = args[0].device
            if device is None or torch.device(device).type != self.device_type:
                return orig(*args, **kwargs)
            if _capturing():
                raise GuardError(f"guarded torch.{name} while a stream is capturing")
            self._tls.busy = True
            try:
                kw = dict(kwargs)
                kw.pop("pin_memory", None)
                req = kw.pop("requires_grad", False)
                kw["device"] = "meta"
                spec = orig(*args, **kw)
                value = None
                if kind == "value":
                    value = kwargs["fill_value"] if "fill_value" in kwargs else args[2 if method else 1]
                t = self._alloc(spec.size(), spec.stride(), spec.dtype, torch.device(device), kind,
                                value, ("Tensor." if method else "torch.") + name)
                return t.requires_grad_(True) if req else t
            finally:
                self._tls.busy = False
        factory.__name__ = name
        return factory

    # -- arenas -----------------------------------------------------------------------------
    def _alloc(self, size, stride, dtype, device, kind, value, what):
        raw_empty = self._orig.get("empty", torch.empty)
        size, stride = tuple(size), tuple(stride)
        nbytes = _span_bytes(size, stride, dtype.itemsize)
        byte = self.fill if _poisoned(dtype) else 0
        raw = raw_empty(BAND + ALIGN + nbytes + BAND, dtype=torch.uint8, device=device)
        lead = BAND + (-(raw.data_ptr() + BAND)) % ALIGN
        raw = raw[:lead + nbytes + BAND]
        raw.fill_(byte)
        flat = raw[lead:lead + nbytes].view(dtype)
        t = flat.as_strided(size, stride)  # keeps the view's own storage offset
        if kind == "zero":
            t.zero_()
        elif kind == "one":
            t.fill_(1)
        elif kind == "value":
            t.fill_(value)
        assert nbytes == 0 or t.data_ptr() % ALIGN == 0
        a = Arena(raw, lead, nbytes, byte, size, dtype, _site(), what)
        with self._lock:
            self.arenas.append(a)
            self.bytes += nbytes
            self._storages[raw.untyped_storage().data_ptr()] = a
        return t

    def put(self, t, device=None):
        """A guarded copy of `t` (same shape, dtype and strides) on `device` (default: the
        context's device type)."""
        device = torch.device(device if device is not None else self.device_type)
        if device.type == "cuda" and device.index is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        if _capturing():
            raise GuardError("guard.put while a stream is capturing")
        raw_like = self._orig.get("empty_like", torch.empty_like)
        self._tls.busy = True
        try:
            spec = raw_like(t.detach(), device="meta")
            g = self._alloc(spec.size(), spec.stride(), spec.dtype, device, "poison", None, "guard.put")
            g.copy_(t.detach())
        finally:
            self._tls.busy = False
        return g

    def owns(self, t):
        return isinstance(t, torch.Tensor) and t.untyped_storage().data_ptr() in self._storages

    def arena_of(self, t):
        return self._storages.get(t.untyped_storage().data_ptr())

    # -- the check --------------------------------------------------------------------------
    def dirty(self):
        """[(arena, side, first dirty offset, last dirty offset)], offsets in bytes from the
        start of that band."""
        if self.device_type == "cuda" and self.arenas:
            torch.cuda.synchronize()  # kernels on side streams included
        flags, idx = [], []
        for a in self.arenas:
            for side, band in a.bands():
                flags.append((band != a.byte).any())
                idx.append((a, side, band))
        if not flags:
            return []
        hit = torch.stack(flags).cpu().tolist()  # one synchronisation for all bands
        out = []
        for h, (a, side, band) in zip(hit, idx):
            if h:
                where = (band != a.byte).nonzero().flatten()
                out.append((a, side, int(where[0]), int(where[-1])))
        return out

    def check(self):
        bad = self.dirty()
        if bad:
            lines = [f"{len(bad)} guard band(s) overwritten (fill 0x{self.fill:02X}):"]
            for a, side, lo, hi in bad[:20]:
                rel = (f"{lo - a.lead} .. {hi - a.lead} bytes relative to the payload start"
                       if side == "leading" else
                       f"{lo} .. {hi} bytes past the payload end")
                lines.append(f"  {a.describe()}: {side} band, dirty offsets {lo} .. {hi} ({rel}), "
                             f"payload {a.nbytes} bytes")
            raise GuardError("\n".join(lines))

    def stats(self):
        return len(self.arenas), self.bytes


def put(t, device="cuda"):
    """Inside a context: a guarded copy of `t`.  Outside: a plain fresh copy on `device`."""
    if _active is not None:
        return _active.put(t, device if _active.device_type != "cpu" else "cpu")
    return t.detach().to(device, copy=True)


def owns(t):
    ctx = _active or _last
    return ctx is not None and ctx.owns(t)


def active():
    return _active
