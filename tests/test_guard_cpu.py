"""tests/guard.py, the guarded-allocation harness, exercised on CPU tensors: fidelity against the
original factories, prefill and poison, reporting of seeded host-side overruns (plain tensor
indexing on the arena, not a kernel), a clean run, and restoration of the factories."""
import pytest
import torch

import guard

CPU = dict(device="cpu")
CL = torch.channels_last


def _like_sources():
    base = torch.arange(2 * 6 * 5 * 4, dtype=torch.float32).view(2, 6, 5, 4)
    return {
        "contiguous": base,
        "channels_last": base.contiguous(memory_format=CL),
        "sliced_channels": base[:, 1:4],
        "sliced_width": base[..., 1:3],
        "bev_bstride": base.view(2, -1)[:, :7],
        "transposed": base.transpose(1, 3),
        "zero_elements": base[:, :0],
        "int64": torch.arange(12).view(3, 4)[:, 1:],
    }


# (factory name, args, kwargs); every call also gets device="cpu"
CALLS = [
    ("empty", (3, 5), {}),
    ("empty", ((3, 5),), {}),
    ("empty", (7,), dict(dtype=torch.float64)),
    ("empty", (2, 3, 4, 5), dict(dtype=torch.bfloat16)),
    ("empty", ((4, 1),), dict(dtype=torch.int32)),
    ("empty", (1027,), dict(dtype=torch.uint8)),
    ("empty", ((),), dict(dtype=torch.int64)),
    ("empty", (2, 6, 5, 4), dict(memory_format=CL)),
    ("empty", ((2, 6, 5, 4),), dict(memory_format=CL, dtype=torch.bfloat16)),
    ("empty", (0,), {}),
    ("empty", (3, 0, 2), dict(dtype=torch.int64)),
    ("zeros", (3, 5), {}),
    ("zeros", ((2, 3, 4),), dict(dtype=torch.float64)),
    ("zeros", (5,), dict(dtype=torch.int32)),
    ("zeros", ((),), dict(dtype=torch.int64)),
    ("zeros", (0, 4), dict(dtype=torch.uint8)),
    ("ones", (3, 5), {}),
    ("ones", ((6,),), dict(dtype=torch.bfloat16)),
    ("ones", (2, 2), dict(dtype=torch.int64)),
    ("full", ((3, 5), 2.5), {}),
    ("full", ((), 7), dict(dtype=torch.int64)),
    ("full", ((4,), float("nan")), {}),
    ("full", ((2, 3),), dict(fill_value=3, dtype=torch.uint8)),
    ("full", ((0,), 1.0), dict(dtype=torch.float64)),
]


@pytest.mark.parametrize("fill", [guard.FILL_A, guard.FILL_B], ids=["fillA", "fillB"])
@pytest.mark.parametrize("name,args,kwargs", CALLS, ids=[f"{i}-{c[0]}" for i, c in enumerate(CALLS)])
def test_factories_match_the_originals(name, args, kwargs, fill):
    ref = getattr(torch, name)(*args, **kwargs, **CPU)
    with guard.allocations(fill, device_type="cpu") as g:
        t = getattr(torch, name)(*args, **kwargs, **CPU)
        assert g.owns(t) and guard.owns(t)
        g.check()
    _same_layout(t, ref)
    _prefill(name, t, ref, fill)
    _placed(g, t)


@pytest.mark.parametrize("fill", [guard.FILL_A, guard.FILL_B], ids=["fillA", "fillB"])
@pytest.mark.parametrize("src", list(_like_sources()))
@pytest.mark.parametrize("name", ["empty_like", "zeros_like", "ones_like", "full_like"])
def test_like_factories_match_the_originals(name, src, fill):
    x = _like_sources()[src]
    extra = (3,) if name == "full_like" else ()
    for kwargs in ({}, dict(dtype=torch.float64), dict(memory_format=torch.contiguous_format)):
        ref = getattr(torch, name)(x, *extra, **kwargs)
        with guard.allocations(fill, device_type="cpu") as g:
            t = getattr(torch, name)(x, *extra, **kwargs)
            assert g.owns(t)
            g.check()
        _same_layout(t, ref)
        _prefill(name, t, ref, fill)
        _placed(g, t)


@pytest.mark.parametrize("name,args", [("new_empty", ((3, 2),)), ("new_zeros", ((3, 2),)),
                                       ("new_ones", (4,)), ("new_full", ((2, 2), 5.0))])
def test_new_methods_match_the_originals(name, args):
    x = torch.randn(5, dtype=torch.float64)
    ref = getattr(x, name)(*args)
    with guard.allocations(guard.FILL_A, device_type="cpu") as g:
        t = getattr(x, name)(*args)
        assert g.owns(t)
        g.check()
    _same_layout(t, ref)
    _prefill(name.replace("new_", ""), t, ref, guard.FILL_A)


def _same_layout(t, ref):
    assert t.shape == ref.shape and t.dtype == ref.dtype and t.device == ref.device
    assert t.stride() == ref.stride(), (t.stride(), ref.stride())
    assert t.requires_grad == ref.requires_grad


def _prefill(name, t, ref, fill):
    if name.startswith("empty"):
        if t.numel() == 0:
            return
        byte = fill if guard._poisoned(t.dtype) else 0
        a = guard._last.arena_of(t)
        assert bool((a.raw[a.lead:a.lead + a.nbytes] == byte).all())
        if t.dtype.is_floating_point:
            v = t.double()
            if fill == guard.FILL_A:
                assert bool(torch.isnan(v).all())
            else:
                assert bool(torch.isfinite(v).all()) and bool((v > 1e38).all() or t.dtype == torch.float64)
    else:
        assert torch.equal(t, ref) or (t.dtype.is_floating_point and bool(torch.isnan(ref).all())
                                       and bool(torch.isnan(t).all()))


def _placed(g, t):
    """The payload is 512-B aligned, spans exactly the tensor's bytes, and the trailing band
    starts at the very next byte; both bands are at least 64 KiB."""
    a = g.arena_of(t)
    assert a.nbytes == guard._span_bytes(t.shape, t.stride(), t.element_size())
    assert (a.raw.data_ptr() + a.lead) % guard.ALIGN == 0
    if t.numel():
        assert t.data_ptr() == a.raw.data_ptr() + a.lead
    (_, lead), (_, trail) = a.bands()
    assert lead.numel() >= guard.BAND and trail.numel() == guard.BAND
    assert trail.data_ptr() == a.raw.data_ptr() + a.lead + a.nbytes


def test_span_of_a_strided_like_is_exact():
    x = torch.zeros(4, 10)[:, :3].t()  # empty_like gives a dense (3, 4) in the source's order
    with guard.allocations(guard.FILL_B, device_type="cpu") as g:
        t = torch.empty_like(x)
        assert g.arena_of(t).nbytes == 12 * 4
        g.check()
    assert t.stride() == torch.empty_like(x).stride()


def test_other_devices_and_out_pass_through():
    with guard.allocations(guard.FILL_A, device_type="cuda") as g:
        a = torch.empty(3, device="cpu")
        b = torch.zeros(3)
        c = torch.empty_like(b)
        d = torch.full((2,), 1.0, device="meta")
        assert not any(g.owns(t) for t in (a, b, c, d)) and g.stats() == (0, 0)
        g.check()
    with guard.allocations(guard.FILL_A, device_type="cpu") as g:
        buf = torch.empty(3)  # no device given: untouched
        assert not g.owns(buf)
        e = torch.zeros(3, device="cpu", out=buf)
        assert e.data_ptr() == buf.data_ptr() and not g.owns(e)


def test_put_copies_values_layout_and_is_plain_outside():
    src = _like_sources()
    strides = {k: torch.empty_like(x).stride() for k, x in src.items()}
    with guard.allocations(guard.FILL_A, device_type="cpu") as g:
        for k, x in src.items():
            t = guard.put(x)
            assert g.owns(t) and torch.equal(t, x), k
            assert t.stride() == strides[k] and t.dtype == x.dtype
        p = torch.nn.Parameter(torch.randn(5, 3))
        before = p.detach().clone()
        p.data = guard.put(p.data)
        assert g.owns(p) and torch.equal(p.detach(), before) and p.requires_grad
        n, nbytes = g.stats()
        assert n == len(src) + 1 and nbytes > 0
        g.check()
    x = src["contiguous"]
    t = guard.put(x, "cpu")
    assert torch.equal(t, x) and t.data_ptr() != x.data_ptr() and not guard.owns(t)


@pytest.mark.parametrize("fill", [guard.FILL_A, guard.FILL_B], ids=["fillA", "fillB"])
@pytest.mark.parametrize("where", ["one_past_end", "one_before_start", "last_trailing_byte"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int64, torch.uint8])
def test_host_overrun_is_reported(where, fill, dtype):
    """One stray byte, written by plain tensor indexing on the arena, is reported with the
    tensor (shape, dtype, allocating line), the side and the offset; its neighbours stay
    clean."""
    with guard.allocations(fill, device_type="cpu") as g:
        before = torch.zeros(9, **CPU)
        victim = torch.empty(3, 5, dtype=dtype, **CPU); line = _line()  # noqa: E702
        after = torch.empty(11, dtype=torch.float64, **CPU)
        a = g.arena_of(victim)
        end = a.lead + a.nbytes
        pos, side, off = {"one_past_end": (end, "trailing", 0),
                          "one_before_start": (a.lead - 1, "leading", a.lead - 1),
                          "last_trailing_byte": (end + guard.BAND - 1, "trailing", guard.BAND - 1)}[where]
        a.raw[pos] = a.byte ^ 0x5A
        assert g.dirty() == [(a, side, off, off)]
        with pytest.raises(guard.GuardError) as e:
            g.check()
        msg = str(e.value)
        assert "1 guard band(s)" in msg and f"{side} band" in msg
        assert f"(3, 5) {dtype}" in msg and f"{__file__}:{line}" in msg
        assert f"dirty offsets {off} .. {off}" in msg
        assert g.owns(before) and g.owns(after)
        # a two-byte run: first and last offsets
        a.raw[end + 100] = a.byte ^ 1
        if where == "one_past_end":
            assert g.dirty() == [(a, "trailing", 0, 100)]
        a.raw[pos] = a.byte
        a.raw[end + 100] = a.byte
        g.check()


def _line():
    import sys
    return sys._getframe(1).f_lineno


def test_writes_inside_the_payload_are_clean():
    with guard.allocations(guard.FILL_A, device_type="cpu") as g:
        ts = [torch.empty(3, 5, **CPU), torch.zeros(7, dtype=torch.int32, **CPU),
              torch.empty(2, 6, 5, 4, memory_format=CL, **CPU), torch.empty(0, **CPU),
              torch.empty(1027, dtype=torch.uint8, **CPU)]
        for t in ts:
            t.fill_(1)
        ts[0][-1, -1] = 2.0
        ts[4][-1] = 3
        g.check()
        assert g.stats()[0] == 5


def test_factories_are_restored_after_an_exception():
    names = list(guard._FACTORIES)
    orig = {n: getattr(torch, n) for n in names}
    orig_m = {n: getattr(torch.Tensor, n) for n in guard._METHODS}
    with pytest.raises(RuntimeError, match="boom"):
        with guard.allocations(guard.FILL_B, device_type="cpu"):
            assert all(getattr(torch, n) is not orig[n] for n in names)
            raise RuntimeError("boom")
    assert all(getattr(torch, n) is orig[n] for n in names)
    assert all(getattr(torch.Tensor, n) is orig_m[n] for n in guard._METHODS)
    assert guard.active() is None
    with guard.allocations(guard.FILL_B, device_type="cpu"):  # and a new context starts
        with pytest.raises(guard.GuardError, match="nest"):
            with guard.allocations(guard.FILL_A, device_type="cpu"):
                pass
    assert all(getattr(torch, n) is orig[n] for n in names)


def test_requires_grad_and_autograd_through_guarded_tensors():
    with guard.allocations(guard.FILL_A, device_type="cpu") as g:
        w = torch.ones(4, requires_grad=True, **CPU)
        assert w.requires_grad and w.is_leaf and g.owns(w)
        (w * 3).sum().backward()
        assert torch.equal(w.grad, torch.full((4,), 3.0))
        g.check()
