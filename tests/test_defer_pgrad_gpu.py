"""Deferred parameter-gradient finishing (e2ep_amd.defer, csrc/pgrad.hip, e2ep_tune key 37).

Inside a defer.ParamGradDefer scope the split-slab sum of a conv weight gradient, the
LayerNorm dgamma / dbeta partial sum and the squeeze-excitation weight gradient are recorded
and run batched at the scope's exit.  A block of a batched kernel runs the same device function
as a block of the launch it replaces, so every result must equal the immediate one BIT FOR BIT
(torch.equal throughout)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (N, Cin, H, W, Cout, R, S, stride, pad, dilation)
# the six small geometries of tests/test_splitk_fold_gpu.py::CONV (small grids: the plans split K)
FOLD = [(2, 160, 8, 8, 960, 1, 1, 1, 0, 1), (4, 320, 16, 16, 64, 1, 1, 1, 0, 1),
        (2, 64, 16, 16, 64, 3, 3, 1, 1, 1), (2, 256, 8, 8, 256, 3, 3, 1, 1, 1),
        (3, 100, 8, 8, 70, 1, 1, 1, 0, 1), (1, 216, 12, 12, 48, 3, 3, 1, 1, 1)]
F4 = (2, 256, 8, 8, 256, 3, 3, 1, 1, 1)     # n = 589 824: the float4 flavour (splits <= 64)
DEAD = (2, 32, 8, 8, 32, 3, 3, 1, 8, 8)     # dilation = map size: only the centre tap is live
ODD = (1, 7, 5, 5, 9, 3, 3, 1, 1, 1)        # n = 567: no multiple of 64 (nor of 4)
MANY = (8, 32, 32, 32, 32, 1, 1, 1, 0, 1)   # 8192 pixels: tens of slabs on the 16-lane flavour
TINY = (1, 8, 4, 4, 8, 1, 1, 1, 0, 1)       # n = 64, one block


def _dims(case):
    N, Cin, H, W, Cout, R, S, st, p, d = case
    P = (H + 2 * p - d * (R - 1) - 1) // st + 1
    Q = (W + 2 * p - d * (S - 1) - 1) // st + 1
    return (N, Cin, H, W, Cout, R, S, P, Q, st, st, p, p, d, d)


def _splits(case):
    from e2ep_amd import _lib
    return _lib.load().e2ep_conv_wgrad_splits(_lib.dims(_dims(case)))


def _inputs(case, seed=0):
    N, Cin, H, W, Cout, R, S = case[:7]
    d = _dims(case)
    g = torch.Generator().manual_seed(seed + N * 31 + Cin + Cout)
    x = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    gy = torch.randn(N, Cout, d[7], d[8], generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, R, S, generator=g) / (Cin * R * S) ** 0.5).to(DEV)
    return x, gy, w


def _wgrad(case, x, gy, fill_ws=None, accumulate=0, dw=None):
    """e2ep_conv_wgrad through conv.conv_wgrad (accumulate = 0) or the entry point itself."""
    from e2ep_amd import _lib, conv, defer
    d = _dims(case)
    N, Cin, H, W, Cout, R, S = case[:7]
    if dw is None:
        dw = torch.empty(Cout, Cin, R, S, device=DEV)
    ws = torch.empty(_splits(case) * dw.numel(), device=DEV)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    if not accumulate:
        return conv.conv_wgrad(gy, x, d, dw, ws)
    with defer.call() as dc:
        dc.keep(ws)
        _lib.call("e2ep_conv_wgrad", _lib.ptr(gy), _lib.ptr(x), _lib.dims(d), _splits(case),
                  _lib.ptr(ws), _lib.nbytes(ws), _lib.ptr(dw), accumulate, _lib.stream(), 0)
    return dw


def _pair_ok(case):
    from e2ep_amd import _lib
    return _lib.load().e2ep_conv_bwd_pair_ok(_lib.dims(_dims(case)), case[1]) == 1


def _pair(case, x, gy, w):
    """(dx, dw) through e2ep_conv_bwd, deferring whenever a scope is open."""
    from e2ep_amd import conv, defer
    return conv._conv_bwd_pair(gy, x, conv.tap_major(w), _dims(case), case[1], None, w.shape,
                               defer.ANY)


def _run_mix(cases, data):
    """Every case's weight gradient, and its paired backward where the plan has one."""
    out = []
    for c, (x, gy, w) in zip(cases, data):
        out.append(_wgrad(c, x, gy))
        if _pair_ok(c):
            out.extend(_pair(c, x, gy, w))
    return out


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_conv_slabs_deferred_equal_immediate(prec):
    """All the geometries in ONE scope, so its launch holds records of both flavours, many
    and single splits, an n that is no multiple of 64, and dead taps."""
    from e2ep_amd import _lib, defer, precision
    cases = FOLD + [DEAD, ODD, MANY, TINY]
    data = [_inputs(c) for c in cases]
    with precision.use(prec):
        n4 = F4[4] * F4[1] * F4[5] * F4[6]
        assert n4 == 589824 and _splits(F4) <= 64          # the float4 flavour's conditions
        assert _splits(MANY) > 16 and MANY[4] * MANY[1] < 131072  # many slabs, 16-lane flavour
        assert min(_splits(c) for c in cases) == 1         # a single split is among them
        ref = _run_mix(cases, data)
        with defer.ParamGradDefer():
            got = _run_mix(cases, data)
            assert _lib.call_raw("e2ep_defer_pending") >= len(cases)
        assert _lib.call_raw("e2ep_defer_pending") == 0
        torch.cuda.synchronize()
    assert len(ref) == len(got) > len(cases)  # some pairs ran
    for i, (a, b) in enumerate(zip(ref, got)):
        assert torch.equal(a, b), (prec, i)


def test_dead_taps_written_as_zeros():
    """A 3x3 whose dilation is the map size (the ASPP branches): the GEMM never writes the eight
    dead taps' slab entries (left NaN here); the sum writes zeros there, both ways."""
    from e2ep_amd import defer
    x, gy, _ = _inputs(DEAD)
    ref = _wgrad(DEAD, x, gy, fill_ws=float("nan"))
    with defer.ParamGradDefer():
        got = _wgrad(DEAD, x, gy, fill_ws=float("nan"))
    live = torch.zeros(3, 3, dtype=torch.bool, device=DEV)
    live[1, 1] = True
    assert (ref[:, :, ~live] == 0).all() and ref[:, :, 1, 1].abs().max() > 0
    assert torch.isfinite(ref).all()
    assert torch.equal(ref, got)


@pytest.mark.parametrize("case", [FOLD[1], F4], ids=["lanes16", "float4"])
def test_accumulate_into_prefilled_gradient(case):
    """accumulate = 1 into a pre-filled dw, then a second accumulating record of the same dw
    in the same scope (it must see the first one's result: the flush orders them)."""
    from e2ep_amd import defer
    x, gy, _ = _inputs(case)
    x2, gy2, _ = _inputs(case, seed=5)
    N, Cin, H, W, Cout, R, S = case[:7]
    fill = torch.randn(Cout, Cin, R, S, generator=torch.Generator().manual_seed(3)).to(DEV)

    def run():
        dw = fill.clone()
        _wgrad(case, x, gy, accumulate=1, dw=dw)
        _wgrad(case, x2, gy2, accumulate=1, dw=dw)
        return dw

    ref = run()
    with defer.ParamGradDefer():
        got = run()
    assert not torch.equal(ref, fill)
    assert torch.equal(ref, got)


def test_more_records_than_one_launch():
    """150 tiny 1x1 weight gradients in one scope (a launch's arguments hold 64 records)."""
    from e2ep_amd import _lib, defer
    data = [_inputs(TINY, seed=i) for i in range(150)]
    ref = [_wgrad(TINY, x, gy) for x, gy, _ in data]
    with defer.ParamGradDefer():
        got = [_wgrad(TINY, x, gy) for x, gy, _ in data]
        assert _lib.call_raw("e2ep_defer_pending") == 150
    assert _lib.call_raw("e2ep_defer_pending") == 0
    for a, b in zip(ref, got):
        assert torch.equal(a, b)


def _grads(fn, params, scope, k=1.0):
    """.grad of every parameter after fn(k) forward + backward (k scales the incoming gradient),
    inside a scope or not."""
    from e2ep_amd import defer
    for p in params:
        p.grad = None
    if scope:
        with defer.ParamGradDefer():
            fn(k)
    else:
        fn(k)
    return [None if p.grad is None else p.grad.clone() for p in params]


def _ref_then_scoped(fn, params):
    """Immediate reference, then a run with another incoming gradient, then the scoped run: a
    gradient tensor the scoped run left unwritten (or that autograd cloned before the flush)
    would hold the middle run's values out of the allocator's cache, not the reference's."""
    ref = _grads(fn, params, False)
    _grads(fn, params, False, k=3.0)
    return ref, _grads(fn, params, True)


@pytest.mark.parametrize("rows", [112, 2048])
@pytest.mark.parametrize("dbeta", [True, False])
def test_layer_norm_param_grads(rows, dbeta):
    from e2ep_amd import _lib, nn_ops
    E = 258
    g = torch.Generator().manual_seed(rows)
    a = torch.randn(rows, E, generator=g).to(DEV).requires_grad_(True)
    b = torch.randn(rows, E, generator=g).to(DEV)
    dy = torch.randn(rows, E, generator=g).to(DEV)
    norm = torch.nn.LayerNorm(E).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(E, generator=g))
    norm.bias.requires_grad_(dbeta)
    params = [norm.weight, norm.bias]
    seen = []

    def fn(k):
        a.grad = None
        nn_ops.add_drop_layer_norm(a, b, norm).backward(dy * k)
        seen.append(_lib.call_raw("e2ep_defer_pending"))

    ref, got = _ref_then_scoped(fn, params)
    assert seen == [0, 0, 1]  # the scoped run really deferred its partial sum
    assert ref[0] is not None and (ref[1] is not None) == dbeta
    for r, o in zip(ref, got):
        assert (r is None and o is None) or torch.equal(r, o)


@pytest.mark.parametrize("shape", [(2, 24, 6), (32, 960, 40)])
def test_se_weight_grads(shape):
    from e2ep_amd import _lib, nn_ops
    N, C, sq = shape
    g = torch.Generator().manual_seed(C)
    x = torch.randn(N, C, 4, 4, generator=g).to(DEV).requires_grad_(True)
    dy = torch.randn(N, C, 4, 4, generator=g).to(DEV)
    w1 = (torch.randn(sq, C, 1, 1, generator=g) / C ** 0.5).to(DEV).requires_grad_(True)
    b1 = torch.randn(sq, generator=g).to(DEV).requires_grad_(True)
    w2 = (torch.randn(C, sq, 1, 1, generator=g) / sq ** 0.5).to(DEV).requires_grad_(True)
    b2 = torch.randn(C, generator=g).to(DEV).requires_grad_(True)
    params = [w1, b1, w2, b2]
    seen = []

    def fn(k):
        x.grad = None
        nn_ops.squeeze_excite(x, w1, b1, w2, b2).backward(dy * k)
        seen.append(_lib.call_raw("e2ep_defer_pending"))

    ref, got = _ref_then_scoped(fn, params)
    assert seen == [0, 0, 1]
    for r, o in zip(ref, got):
        assert r.abs().max() > 0 and torch.equal(r, o)


def test_key_37_off_launches_immediately():
    """e2ep_tune key 37 = 1: nothing is recorded inside a scope, results as ever."""
    from e2ep_amd import _lib, defer
    x, gy, _ = _inputs(FOLD[2])
    ref = _wgrad(FOLD[2], x, gy)
    prev = _lib.load().e2ep_tune(37, 1)
    try:
        with defer.ParamGradDefer():
            got = _wgrad(FOLD[2], x, gy)
            assert _lib.call_raw("e2ep_defer_pending") == 0
    finally:
        _lib.load().e2ep_tune(37, prev)
    assert torch.equal(ref, got)


def test_abort_launches_nothing_and_next_scope_starts_empty():
    from e2ep_amd import _lib, defer
    x, gy, _ = _inputs(FOLD[2])
    dw = torch.full((64, 64, 3, 3), 7.0, device=DEV)
    with pytest.raises(ZeroDivisionError):
        with defer.ParamGradDefer():
            _wgrad(FOLD[2], x, gy, dw=dw)
            assert _lib.call_raw("e2ep_defer_pending") == 1
            1 / 0
    assert _lib.call_raw("e2ep_defer_pending") == 0
    torch.cuda.synchronize()
    assert (dw == 7.0).all()  # the slab sum never ran
    with defer.ParamGradDefer():
        assert _lib.call_raw("e2ep_defer_pending") == 0
        got = _wgrad(FOLD[2], x, gy)
    assert torch.equal(got, _wgrad(FOLD[2], x, gy))


def test_captured_scope_replays():
    """A scope with three conv backwards captured into a graph: every replay, with changed
    inputs, equals the eager immediate result."""
    from e2ep_amd import defer, graphs
    cases = [FOLD[1], FOLD[2], F4]
    data = [_inputs(c) for c in cases]

    def immediate():
        return [t for c, d in zip(cases, data) for t in _pair(c, *d)]

    def scoped():
        with defer.ParamGradDefer():
            return immediate()

    immediate()  # first launches outside the capture
    torch.cuda.synchronize()
    graph, outs, _ = graphs.capture(scoped)
    for seed in (1, 2):
        for c, d in zip(cases, data):
            for t, new in zip(d, _inputs(c, seed=seed)):
                t.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        ref = immediate()
        for a, b in zip(ref, outs):
            assert torch.equal(a, b), seed
