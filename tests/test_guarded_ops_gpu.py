"""Every kernel family run in guard-banded, poisoned buffers (tests/guard.py).

The rest of the suite hands the kernels tensors straight from the caching allocator, whose
512-byte rounding and recycled memory hide a store past the end of an output or workspace, a
read past the end that reaches the result, and reliance on what torch.empty happens to hold.
Here each case runs three times: unguarded, under fill A (0xFF bytes: NaN) and under fill B
(0x7F bytes: 3.4e38), with identical seeds, and must

  (a) leave every guard band of every tensor allocated during the run untouched,
  (b) give bitwise the same tensors in all three runs (the kernels are deterministic),
  (c) have produced those tensors in guarded arenas (the interception reached the op).

Two kinds of case:

* `run_guarded(fn)` with a `fn` written here, which builds its inputs with guard.put and returns
  the tensors that matter.  Shapes no other test holds to fp64 are compared with fp64 inside
  `fn`, with the bound of that op's existing test.
* `body(module, test, *args)`: an existing test body called as a function inside the context,
  its fixture settings applied by hand.  Its own fp64 / bitwise assertions run in every pass; the
  tensors it hands to its comparison helpers (rel_l2, torch.equal, ...) are recorded at that
  moment and are the "returned tensors" of (b) and (c).  (c) uses what was seen at that moment:
  the compared tensor, or what a clone of it was cloned from, lived in an arena.  Exempt from (c)
  are the host copies a body compares (`y.cpu()`), the second argument of its torch.equal calls
  (its reference) and the tensors a case names in `not_arenas` with the reason.

Inputs.  Whatever puts a tensor on the device besides the patched factories is routed through
guard.put for the duration of a pass (`_routes`: Tensor.to / cuda / clone / contiguous,
torch.randn / rand / randint / tensor / arange / *_like with a device), so the bodies' inputs,
seeds and clones are arenas too.  For the operands that go through `_lib.ptr` this is asserted,
not assumed: every such tensor reaching a kernel outside an autograd backward must live in an
arena (`_audit_ptrs`).  The audit does not see the raw `data_ptr()` values the product packs
into device tables (cat / split channel lists, the BN and counter tables, conv's tap-major
table, FlatAdam's chunk table); those tensors are covered by (a) - (c) only.  Inside a backward the one kind of unguarded tensor is the incoming
gradient that torch's own autograd ops formed in the body (`(y * dy).sum().backward()`).
attention.py hands the kernels K and V as integer addresses inside its key / value operand, so
the audit looks that operand up where `attention._forward` receives it.

Exceptions to "poison must not survive in a returned tensor": none.  No returned or recorded
tensor has a partial-write contract; the incremental decoder's K/V caches (ar_decode.py: rows
t+1.. of a cache are written by later steps) are never returned, only the logits read from them.
"""
import contextlib
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard
from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILLS = (None, guard.FILL_A, guard.FILL_B)
STATS = {}  # family -> [guarded allocations, guarded payload bytes]


# ----------------------------------------------------------------------------------------------
# the engine
# ----------------------------------------------------------------------------------------------
def _reseed():
    """torch's generators and the product's dropout seed pool / step RNG, as a fresh process."""
    from e2ep_amd import rng
    torch.manual_seed(20240607)
    rng.end_step()
    rng._state.clear()


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


_CREATORS = ("randn", "rand", "randint", "tensor", "arange", "randn_like", "rand_like")
AUDIT = []  # (file:line, shape, dtype, in a backward pass) of unguarded tensors handed to _lib.ptr


def _is_cuda(dev):
    return dev is not None and torch.device(dev).type == "cuda"


@contextlib.contextmanager
def _routes():
    """Every way the test bodies (and the product) put a tensor on the device besides the
    factories guard.py patches goes through guard.put: Tensor.to / Tensor.cuda of a host
    tensor, Tensor.clone and a copying Tensor.contiguous of a device tensor, and torch.randn / rand / randint / tensor / arange /
    randn_like / rand_like with a device.  The creating calls draw on the host in all three
    passes (outside a context guard.put is a plain copy), so the passes see the same values.
    Calls that must stay in autograd's graph, and calls during stream capture, pass through."""
    saved = {n: getattr(torch.Tensor, n) for n in ("to", "cuda", "clone", "contiguous")}
    saved_f = {n: getattr(torch, n) for n in _CREATORS}

    def plain(t):
        return not (t.requires_grad and torch.is_grad_enabled()) and not guard._capturing()

    def to(self, *args, **kwargs):
        dev = kwargs.get("device")
        if dev is None and args and isinstance(args[0], (str, torch.device)):
            dev = args[0]
        if self.device.type != "cpu" or not _is_cuda(dev) or guard.active() is None or not plain(self):
            return saved["to"](self, *args, **kwargs)
        args = tuple("cpu" if a is dev else a for a in args)
        if "device" in kwargs:
            kwargs = dict(kwargs, device="cpu")
        kwargs.pop("non_blocking", None)
        return guard.put(saved["to"](self, *args, **kwargs), dev)

    def cuda(self, *args, **kwargs):
        if self.device.type != "cpu" or guard.active() is None or not plain(self):
            return saved["cuda"](self, *args, **kwargs)
        return guard.put(self, DEV)

    def clone(self, *args, **kwargs):
        if self.device.type != "cuda" or args or kwargs or guard.active() is None or not plain(self):
            return saved["clone"](self, *args, **kwargs)
        c = guard.put(self, self.device)
        c._of_unguarded = not guard.owns(self) or getattr(self, "_of_unguarded", False)  # for (c)
        return c

    def contiguous(self, *args, **kwargs):
        fmt = kwargs.get("memory_format", args[0] if args else torch.contiguous_format)
        if (self.device.type != "cuda" or guard.active() is None or not plain(self)
                or fmt == torch.preserve_format or self.is_contiguous(memory_format=fmt)):
            return saved["contiguous"](self, *args, **kwargs)
        return torch.empty(self.shape, dtype=self.dtype, device=self.device, memory_format=fmt).copy_(self)

    def creator(name):
        orig = saved_f[name]

        def create(*args, **kwargs):
            dev = kwargs.get("device")
            if dev is None and name.endswith("_like") and args and args[0].is_cuda:
                dev = args[0].device
            gen = kwargs.get("generator")
            if not _is_cuda(dev) or guard._capturing() or (gen is not None and gen.device.type != "cpu"):
                return orig(*args, **kwargs)
            kw = dict(kwargs, device="cpu")
            req = kw.pop("requires_grad", False)
            if name == "tensor" and args and torch.is_tensor(args[0]) and args[0].is_cuda:
                return orig(*args, **kwargs)
            t = guard.put(orig(*args, **kw), dev)
            return t.requires_grad_(True) if req else t
        return create

    for n, f in (("to", to), ("cuda", cuda), ("clone", clone), ("contiguous", contiguous)):
        setattr(torch.Tensor, n, f)
    for n in _CREATORS:
        setattr(torch, n, creator(n))
    try:
        yield
    finally:
        for n, f in saved.items():
            setattr(torch.Tensor, n, f)
        for n, f in saved_f.items():
            setattr(torch, n, f)


@contextlib.contextmanager
def _audit_ptrs():
    """Under the guard: every device tensor whose pointer goes to a kernel through _lib.ptr is
    looked up; the unguarded ones are listed in AUDIT.  run_guarded lets none pass outside an
    autograd backward; inside one, the gradients that torch's own ops formed on the way
    ((y * dy).sum().backward() hands the op dy * 1) are no arena's."""
    import sys
    from e2ep_amd import _lib
    orig = _lib.ptr
    del AUDIT[:]

    def ptr(t):
        if t is not None and t.is_cuda and not guard.owns(t):
            f = sys._getframe(1)
            AUDIT.append((f"{f.f_code.co_filename.rsplit('/', 1)[-1]}:{f.f_lineno}", tuple(t.shape), t.dtype,
                          torch._C._current_graph_task_id() != -1))  # private: "in a backward pass"
        return orig(t)

    from e2ep_amd import attention
    forward = attention._forward

    def attn_forward(qb, kvb, *args, **kwargs):  # K | V go to the kernel as integer addresses
        ptr(kvb)
        return forward(qb, kvb, *args, **kwargs)

    _lib.ptr, attention._forward = ptr, attn_forward
    try:
        yield
    finally:
        _lib.ptr, attention._forward = orig, forward


def _flatten(res, prefix=""):
    if torch.is_tensor(res):
        return [(prefix or "out", res)]
    if isinstance(res, dict):
        return [kv for k, v in res.items() for kv in _flatten(v, f"{prefix}{k}.")]
    if isinstance(res, (list, tuple)):
        return [kv for i, v in enumerate(res) for kv in _flatten(v, f"{prefix}{i}.")]
    assert res is None or isinstance(res, (int, float, bool, str)), type(res)
    return []


def _owned(g, t):
    """(c) for one returned or recorded tensor: what body() saw when the body compared it, else
    whether it lives in an arena; a routed clone counts as what it was cloned from."""
    if hasattr(t, "_was_owned"):
        return t._was_owned
    return g.owns(t) and not getattr(t, "_of_unguarded", False)


def run_guarded(fn, family, strict_owns=True, not_arenas=()):
    """Run `fn` unguarded, under fill A and under fill B; assert (a), (b), (c) and that every
    tensor handed to a kernel outside a backward pass lives in an arena.  strict_owns=False (the
    borrowed bodies) exempts from (c) the host copies a body compares and the second argument
    of its torch.equal calls (its reference, often a torch op's output); `not_arenas` names
    further recorded tensors that by the op's contract no kernel of the product allocates."""
    runs = []
    for fill in FILLS:
        _reseed()
        if fill is None:
            with _routes():
                res = fn()
            torch.cuda.synchronize()
            runs.append([(k, _bits(t), t.dtype, tuple(t.shape), None) for k, t in _flatten(res)])
            continue
        with guard.allocations(fill) as g, _routes(), _audit_ptrs():
            res = fn()
            torch.cuda.synchronize()
            stray = sorted(set(a[:3] for a in AUDIT if not a[3]))
            assert not stray, f"unguarded tensors reached a kernel: {stray}"
            snap = [(k, _bits(t), t.dtype, tuple(t.shape), _owned(g, t), getattr(t, "_exempt", False))
                    for k, t in _flatten(res)]
            g.check()                                                               # (a)
        n, nbytes = g.stats()
        s = STATS.setdefault(family, [0, 0])
        s[0], s[1] = s[0] + n, s[1] + nbytes
        assert n > 0, "nothing was allocated under the guard"
        missing = [k for k, *_, owned, host in snap
                   if not owned and not (host and not strict_owns) and k not in not_arenas]
        assert all(k in [r[0] for r in snap] for k in not_arenas), not_arenas
        assert not missing, f"not in an arena: {missing}"                          # (c)
        assert any(guard.PRODUCT in a.site for a in g.arenas) or any(o for *_, o, _ in snap), \
            "the interception did not reach the op"
        runs.append([r[:5] for r in snap])
        del res
    base = runs[0]
    assert base, "the case returned no tensor"
    for fill, run in zip(FILLS[1:], runs[1:]):
        assert [r[0] for r in run] == [r[0] for r in base], "the passes returned different sets"
        for (k, b0, dt0, sh0, _), (_, b1, dt1, sh1, _) in zip(base, run):
            assert dt0 == dt1 and sh0 == sh1, (k, dt0, dt1, sh0, sh1)
            if not torch.equal(b0, b1):                                             # (b)
                bad = (b0 != b1).nonzero().flatten()
                raise AssertionError(
                    f"{k} {sh0} {dt0}: fill 0x{fill:02X} differs from the unguarded run in {bad.numel()} "
                    f"bytes, first at byte {int(bad[0])}, last at byte {int(bad[-1])}")


def body(module, test, *args, comparers=("rel_l2", "max_scaled"), settings=()):
    """`fn` for run_guarded out of an existing test body: module.test(*args) with `settings`
    (context managers) applied, recording every device or host tensor the body passes to its
    comparison helpers (first argument: the value under test) and to torch.equal (both)."""
    def fn():
        mod = importlib.import_module(module)
        rec = []

        def snap(t):
            if isinstance(t, dict):  # test_agent_post_gpu._run: host arrays by name
                for v in t.values():
                    snap(v)
            elif isinstance(t, np.ndarray):
                c = torch.from_numpy(np.ascontiguousarray(t))
                c._exempt = True
                rec.append(c)
            elif torch.is_tensor(t):
                c = t.detach().clone()  # the body may overwrite or free it later
                c._was_owned = guard.owns(t) and not getattr(t, "_of_unguarded", False)
                c._exempt = not t.is_cuda
                rec.append(c)

        saved = {}
        for name in comparers:
            if hasattr(mod, name):
                orig = saved[name] = getattr(mod, name)

                def wrapped(a, *rest, _orig=orig, **kw):
                    snap(a)
                    return _orig(a, *rest, **kw)
                setattr(mod, name, wrapped)
        equal = torch.equal

        def rec_equal(a, b):
            snap(a)
            n = len(rec)
            snap(b)
            for c in rec[n:]:  # the second argument is the body's reference: in (b), not in (c)
                c._exempt = c._exempt or not c._was_owned
            return equal(a, b)

        torch.equal = rec_equal
        try:
            with contextlib.ExitStack() as st:
                for s in settings:
                    st.enter_context(s())
                getattr(mod, test)(*args)
        finally:
            torch.equal = equal
            for name, orig in saved.items():
                setattr(mod, name, orig)
        return rec
    return fn


def tune(key, value):
    @contextlib.contextmanager
    def cm():
        from e2ep_amd import _lib
        prev = _lib.load().e2ep_tune(key, value)
        try:
            yield
        finally:
            _lib.load().e2ep_tune(key, prev)
    return cm


def raw(name, value):
    """An entry point that sets a value and returns the previous one (e2ep_bn_small, ...)."""
    @contextlib.contextmanager
    def cm():
        from e2ep_amd import _lib
        prev = _lib.call_raw(name, value)
        try:
            yield
        finally:
            _lib.call_raw(name, prev)
    return cm


def setter(module, name, value):
    """A Python-level switch module.name(value) -> previous value (nn_ops.set_dw_pair, ...)."""
    @contextlib.contextmanager
    def cm():
        fn = getattr(importlib.import_module(module), name)
        prev = fn(value)
        try:
            yield
        finally:
            fn(prev)
    return cm


def _ids(cases):
    return [str(i) for i in range(len(cases))]


def _put(t, grad=False):
    t = guard.put(t, DEV)
    return t.requires_grad_(True) if grad else t


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------
# the engine on the device: what it must report, it reports
# ----------------------------------------------------------------------------------------------
def test_engine_reports_device_overruns_and_surviving_poison():
    """Stray writes made with plain tensor indexing inside the arena (no kernel, nothing outside
    the allocation): one float after a payload and one before it are named with tensor, side
    and offsets; an output left unwritten fails (b); an unguarded output fails (c)."""
    with guard.allocations(guard.FILL_A) as g:
        t = torch.empty(3, 5, device=DEV)
        w = torch.empty(1027, dtype=torch.uint8, device=DEV)
        k = torch.zeros(4, dtype=torch.int32, device=DEV)
        assert t.data_ptr() % 512 == 0 and w.data_ptr() % 512 == 0 and bool(torch.isnan(t).all())
        assert bool((w == 0xFF).all()) and int(k.sum()) == 0
        g.check()
        t.as_strided((16,), (1,))[15] = 1.0                      # one float past the end
        a = g.arena_of(w)
        a.raw[a.lead - 1] = 0                                    # the byte before the payload
        bad = g.dirty()
        assert [(x.shape, side, lo, hi) for x, side, lo, hi in bad] == [
            ((3, 5), "trailing", 0, 3), ((1027,), "leading", a.lead - 1, a.lead - 1)]
        with pytest.raises(guard.GuardError, match=r"\(3, 5\) torch.float32.*trailing band, dirty offsets 0 .. 3"):
            g.check()
    with pytest.raises(AssertionError, match="differs from the unguarded run"):
        run_guarded(lambda: torch.empty(8, device=DEV), "engine")  # fill A vs B vs allocator
    with pytest.raises(AssertionError):
        run_guarded(lambda: torch.zeros(8, device=DEV) + 1, "engine")  # a torch op's output: not owned
    for clone in (False, True):  # a borrowed body that compares a torch op's output, or its clone
        with pytest.raises(AssertionError, match="not in an arena"):
            run_guarded(body("test_guarded_ops_gpu", "_plain_op_body", clone), "engine", False)
    run_guarded(body("test_guarded_ops_gpu", "_plain_op_body", True, True), "engine", False)
    STATS.pop("engine", None)


def _plain_op_body(clone, guarded=False):
    """What a borrowed body looks like to body(): it compares a device tensor with rel_l2."""
    x = torch.ones(4).to(DEV)
    y = torch.empty_like(x).copy_(x) if guarded else x + 1
    assert rel_l2(y.clone() if clone else y, y.cpu()) == 0.0


def test_engine_refuses_stream_capture():
    """No guarded context starts, and none allocates, while a stream is capturing."""
    buf = torch.zeros(4, device=DEV)
    factory = torch.empty
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with guard.allocations(guard.FILL_A) as g:
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph):
                buf.add_(1.0)
                with pytest.raises(guard.GuardError, match="capturing"):
                    torch.empty(4, device=DEV)
                with pytest.raises(guard.GuardError, match="capturing"):
                    guard.put(torch.ones(4))
        torch.cuda.current_stream().wait_stream(side)
        assert g.stats() == (0, 0)
    second = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(second):
            buf.add_(1.0)
            with pytest.raises(guard.GuardError, match="capturing"):
                guard.allocations(guard.FILL_B).__enter__()
    torch.cuda.current_stream().wait_stream(side)
    assert guard.active() is None and torch.empty is factory
    graph.replay()
    torch.cuda.synchronize()
    assert buf.tolist() == [1.0] * 4


# ----------------------------------------------------------------------------------------------
# resize
# ----------------------------------------------------------------------------------------------
RESIZE = [((3, 5, 17, 9), (40, 7)), ((2, 7, 50, 60), (40, 90)), ((3, 70, 37, 45), (50, 61)),
          ((32, 64, 1, 1), (16, 16))]


@pytest.mark.parametrize("shape,size", RESIZE, ids=_ids(RESIZE))
def test_resize(shape, size):
    run_guarded(body("test_nn_ops_gpu", "test_resize", (shape, size, None)), "resize", False)


@pytest.mark.parametrize("shape,size", RESIZE, ids=_ids(RESIZE))
def test_resize_bwd_channels_last(shape, size):
    """e2ep_resize_bwd_cl serves input / output ratios of at least 0.5 and refuses the rest (the
    first and last entry of RESIZE) with an error before it launches anything; the NCHW backward
    of those two runs in test_resize above."""
    from e2ep_amd import _lib
    fn = body("test_nn_ops_gpu", "test_resize_bwd_channels_last_equals_nchw", *shape, *size)
    if min(shape[2] / size[0], shape[3] / size[1]) < 0.5:
        with pytest.raises(_lib.E2EPError, match="scale < 0.5"):
            fn()
        return
    run_guarded(fn, "resize", False)


# ----------------------------------------------------------------------------------------------
# depthwise convolution
# ----------------------------------------------------------------------------------------------
DW = [(3, 8, 13, 11, 3, 2, (0, 1, 0, 1)), (2, 12, 24, 20, 5, 1, (2, 2, 2, 2)),
      (2, 6, 64, 48, 5, 2, (2, 2, 2, 2)), (2, 16, 32, 32, 5, 1, (3, 1, 3, 1))]
DW_PAIRED = [c for c in DW if c in ((2, 12, 24, 20, 5, 1, (2, 2, 2, 2)), (2, 6, 64, 48, 5, 2, (2, 2, 2, 2)))]


@pytest.mark.parametrize("variant", [(2, 0), (1, 3)], ids=["vec_default", "scalar_grid3"])
@pytest.mark.parametrize("case", DW, ids=_ids(DW))
def test_depthwise(case, variant):
    run_guarded(body("test_nn_ops_gpu", "test_depthwise", case, variant), "depthwise", False)


@pytest.mark.parametrize("fused", [False, True], ids=["dw", "bn_swish_dw"])
@pytest.mark.parametrize("case", DW_PAIRED, ids=_ids(DW_PAIRED))
def test_depthwise_paired_and_forked_backward(case, fused):
    """The members of the issue's list that e2ep_dwconv_bwd_pair_ok accepts (the body asserts
    it): paired launch and forked dgrad + wgrad."""
    run_guarded(body("test_nn_ops_gpu", "test_depthwise_bwd_pair_bitwise_equals_two_launches", case, fused),
                "depthwise", False)


@pytest.mark.parametrize("paths", [(1, None), (0, 3)], ids=["bn_one_launch_grid_default", "bn_split_grid3"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", DW, ids=_ids(DW))
def test_bn_swish_depthwise(case, train, paths):
    bn_small, grid = paths
    settings = [raw("e2ep_bn_small", bn_small)] + ([tune(24, grid)] if grid else [])
    run_guarded(body("test_nn_ops_gpu", "test_bn_swish_depthwise_fused", case + (train,), bn_small, grid or 0,
                     settings=settings), "depthwise", False)


# ----------------------------------------------------------------------------------------------
# BatchNorm
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bn_small", [1, 0], ids=["bn_one_launch", "bn_split"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("act,res", [("swish", True), ("relu", False)])
@pytest.mark.parametrize("shape", [(3, 7, 5, 9), (32, 6, 1, 1), (4, 24, 32, 32)])
def test_bn_act(shape, act, res, train, bn_small):
    run_guarded(body("test_nn_ops_gpu", "test_bn_act", train, act, res, shape, bn_small,
                     settings=[raw("e2ep_bn_small", bn_small)]), "batchnorm", False)


@pytest.mark.parametrize("bn_small", [1, 0], ids=["bn_one_launch", "bn_split"])
def test_bn_drop_connect(bn_small):
    """The third tensor the body compares is the residual's gradient.  Without an activation
    _BatchNormAct.backward returns the incoming gradient itself for it (nn_ops.py: dres_is_dy), so
    autograd's accumulation copies it: no kernel writes it and it is no arena."""
    run_guarded(body("test_nn_ops_gpu", "test_bn_drop_connect_fused", (6, 10, 5, 7), bn_small,
                     settings=[raw("e2ep_bn_small", bn_small)]), "batchnorm", False, not_arenas=("2.",))


# ----------------------------------------------------------------------------------------------
# squeeze-excitation, MBConv middle
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 40, 9, 7, 10), (5, 300, 3, 3, 75)])
def test_squeeze_excite(shape):
    run_guarded(body("test_nn_ops_gpu", "test_squeeze_excite_fused", shape), "squeeze_excite", False)


@pytest.mark.parametrize("bn_small", [1, 0], ids=["bn_one_launch", "bn_split"])
@pytest.mark.parametrize("sums", [True, False], ids=["bn_sums_in_se", "bn_own_reduce"])
def test_bn_swish_se(sums, bn_small):
    run_guarded(body("test_nn_ops_gpu", "test_bn_swish_se_fused", (6, 56, 30, 30, 14, True), bn_small, sums,
                     settings=[raw("e2ep_bn_small", bn_small), setter("e2ep_amd.nn_ops", "set_se_bn_sums", sums)]),
                "squeeze_excite", False)


def test_mbconv_mid_smallest():
    run_guarded(body("test_mbconv_mid_gpu", "test_fused_equals_separate", (1, 3, 3),
                     comparers=("rel_l2", "_err")), "mbconv_mid", False)


# ----------------------------------------------------------------------------------------------
# pools and the SE gate
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5, 5, 4), (3, 2, 7, 64)])
def test_pools_and_gate(shape):
    """max_pool3s2, global_avg_pool and se_gate, each alone; fp64 bounds of
    test_maxpool_avgpool_segate (max pool exact, its gradient 1e-7, the others 1e-6)."""
    from e2ep_amd import nn_ops
    N, C = shape[:2]
    g = _g(sum(shape))
    x = torch.randn(*shape, generator=g)
    x[0, 0, :2, :2] = 1.0  # ties: first maximum wins
    a = torch.randn(N, C, 1, 1, generator=g)
    x64 = x.double().requires_grad_(True)
    a64 = a.double().requires_grad_(True)
    yp64 = F.max_pool2d(x64, 3, 2, 1)
    dyp = torch.randn(yp64.shape, generator=g)
    dyg = torch.randn(*shape, generator=g)
    dya = torch.randn(N, C, 1, 1, generator=g)
    yp64.backward(dyp.double())
    gp64, x64.grad = x64.grad, None
    yg64 = x64 * torch.sigmoid(a64)
    yg64.backward(dyg.double())
    gg64, x64.grad = x64.grad, None
    ya64 = x64.mean((2, 3), keepdim=True)
    ya64.backward(dya.double())
    ga64 = x64.grad

    def fn():
        out = {}
        xd = _put(x, True)
        y = nn_ops.max_pool3s2(xd)
        y.backward(_put(dyp))
        out["pool"], out["pool_dx"] = y, xd.grad
        assert torch.equal(y.detach().cpu().double(), yp64.detach()) and rel_l2(xd.grad, gp64) < 1e-7
        xd, ad = _put(x, True), _put(a, True)
        y = nn_ops.se_gate(xd, ad)
        y.backward(_put(dyg))
        out["gate"], out["gate_dx"], out["gate_da"] = y, xd.grad, ad.grad
        assert rel_l2(y, yg64) < 1e-6 and rel_l2(xd.grad, gg64) < 1e-6 and rel_l2(ad.grad, a64.grad) < 1e-6
        xd = _put(x, True)
        y = nn_ops.global_avg_pool(xd)
        y.backward(_put(dya))
        out["avg"], out["avg_dx"] = y, xd.grad
        assert rel_l2(y, ya64) < 1e-6 and rel_l2(xd.grad, ga64) < 1e-6
        return out

    run_guarded(fn, "pools_gate")


# ----------------------------------------------------------------------------------------------
# softmax over channels, cat / split, small kernels
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 1, 4, 4)])
def test_softmax_channels(shape):
    run_guarded(body("test_nn_ops_gpu", "test_softmax_channels_vs_fp64", shape), "softmax_channels", False)


def test_cat_split_channels():
    run_guarded(body("test_nn_ops_gpu", "test_cat_channels_matches_torch", [(3, 56, 32, 32), (3, 160, 32, 32)]),
                "cat_split", False)


def test_sum3_eq_mask_counters():
    """As test_sum3_eq_mask_counters, every operand and the 300 counters in arenas of their own."""
    from e2ep_amd import _lib, nn_ops
    tok = torch.randint(0, 5, (6, 15), generator=_g(3))

    def fn():
        a, b, c = (_put(torch.tensor(v), True) for v in (1.1, 2.0e-7, -3.3))
        s = nn_ops.sum3(a, b, c)
        assert s.item() == ((torch.tensor(1.1) + torch.tensor(2.0e-7)) + torch.tensor(-3.3)).item()
        s.backward()
        assert a.grad.item() == b.grad.item() == c.grad.item() == 1.0
        mask = nn_ops.eq_mask(_put(tok)[:, 1:], 2)
        assert torch.equal(mask.cpu(), tok[:, 1:] == 2)
        ctr = [torch.full((), k, dtype=torch.int64, device=DEV) for k in range(300)]
        table = _put(torch.tensor([t.data_ptr() for t in ctr], dtype=torch.int64))
        _lib.call("e2ep_add_i64_multi", _lib.ptr(table), len(ctr), 1, _lib.stream())
        assert [int(t) for t in ctr] == [k + 1 for k in range(300)]
        return {"sum": s, "mask": mask, "ctr": ctr[:3] + ctr[-3:]}

    run_guarded(fn, "small_kernels")


def test_rng_draw():
    """e2ep_rng_draw into exact-size buffers: 4096 floats in [0, 1), 64 distinct non-negative
    seeds, the state advanced by one per launch (the eager part of test_step_rng_draws)."""
    from e2ep_amd import _lib

    def fn():
        st = _put(torch.tensor([12345, 0], dtype=torch.int64))
        f = torch.empty(4096, device=DEV)
        iv = torch.empty(64, dtype=torch.int32, device=DEV)
        outs = []
        for _ in range(2):
            _lib.call("e2ep_rng_draw", _lib.ptr(st), f.numel(), _lib.ptr(f), iv.numel(), _lib.ptr(iv),
                      _lib.stream())
            outs += [torch.empty_like(f).copy_(f), torch.empty_like(iv).copy_(iv)]
        a, ai = outs[0], outs[1]
        assert 0.0 <= float(a.min()) and float(a.max()) < 1.0 and abs(float(a.mean()) - 0.5) < 0.03
        assert int(ai.min()) >= 0 and len(set(ai.tolist())) == 64
        assert not torch.equal(a, outs[2]) and int(st[1]) == 2
        return outs + [st]

    run_guarded(fn, "small_kernels")


# ----------------------------------------------------------------------------------------------
# add + dropout + LayerNorm, relu + dropout
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,E,p", [(37, 100, 0.5), (7, 33, 0.5), (5, 65, 0.0)])
def test_add_dropout_layernorm(rows, E, p):
    run_guarded(body("test_nn_ops_gpu", "test_add_dropout_layernorm_fused", rows, E, p), "layernorm", False)


@pytest.mark.parametrize("rows,E,p", [(37, 100, 0.5), (7, 33, 0.5)])
def test_add_dropout_layernorm_seeded(rows, E, p):
    run_guarded(body("test_nn_ops_gpu", "test_add_dropout_layernorm_seeded", rows, E, p), "layernorm", False)


def test_relu_dropout_refuses_odd_length():
    """e2ep_relu_dropout_fwd takes a multiple of 4 elements (the FFN width is 2048) and refuses
    any other n with an error, launching nothing."""
    from e2ep_amd import _lib, nn_ops
    with pytest.raises(_lib.E2EPError, match="multiple of 4"):
        nn_ops.relu_dropout(torch.randn(13, 79, device=DEV), 0.0, None)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_relu_dropout_short_tail(p):
    """n = 4 x 257 = 1028: the smallest kind of length the entry point accepts that is no
    multiple of 8, of a wave or of a block; bounds of
    test_relu_dropout_matches_masked_reference (1e-6) with the kernel's own keep mask."""
    from e2ep_amd import _lib, nn_ops
    g = _g(5)
    x, dy = torch.randn(4, 257, generator=g), torch.randn(4, 257, generator=g)
    n = x.numel()

    def fn():
        seed = _put(torch.tensor([777], dtype=torch.int32))
        keep = torch.empty(n, dtype=torch.uint8, device=DEV)
        _lib.call("e2ep_attn_keep_mask", _lib.ptr(seed), 1, 1, n, p, _lib.ptr(keep), _lib.stream())
        k64 = keep.cpu().double().view_as(x)
        xd = _put(x, True)
        y = nn_ops.relu_dropout(xd, p, seed if p > 0 else None)
        y.backward(_put(dy))
        xr = x.double().requires_grad_(True)
        yr = torch.relu(xr) * k64 / (1 - p)
        yr.backward(dy.double())
        assert rel_l2(y, yr) < 1e-6 and rel_l2(xd.grad, xr.grad) < 1e-6
        return {"keep": keep, "y": y, "dx": xd.grad}

    run_guarded(fn, "relu_dropout")


# ----------------------------------------------------------------------------------------------
# e2ep_gemm and the linear built on it
# ----------------------------------------------------------------------------------------------
LAYOUTS = [(True, True), (True, False), (False, False), (False, True)]


@pytest.mark.parametrize("ak,bk", LAYOUTS)
@pytest.mark.parametrize("M,N,K", [(37, 70, 2048), (112, 204, 258)])
def test_gemm_layouts(M, N, K, ak, bk):
    run_guarded(body("test_gemm_gpu", "test_gemm_layouts_vs_fp64", M, N, K, ak, bk), "gemm", False)


@pytest.mark.parametrize("ak,bk", LAYOUTS)
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6])
def test_gemm_every_tile_and_split(tile, ak, bk):
    run_guarded(body("test_gemm_gpu", "test_gemm_every_tile_and_split", tile, ak, bk), "gemm", False)


@pytest.mark.parametrize("rows,N,K", [(37, 70, 100), (24, 64, 15), (300, 33, 64)])
def test_gemm_rowsum(rows, N, K):
    run_guarded(body("test_gemm_gpu", "test_gemm_rowsum_weight_and_bias_gradient", rows, N, K), "gemm", False)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("shape", [(97, 130, 333), (33, 64, 1500)])
def test_linear_bwd_pair(shape, skip, prec):
    run_guarded(body("test_gemm_gpu", "test_linear_bwd_pair_bitwise_equals_two_launches", shape, skip, prec),
                "gemm", False)


@pytest.mark.parametrize("shape,relu,skip", [((8, 14, 258), False, False), ((8, 1, 3), True, False)])
def test_linear_autograd(shape, relu, skip):
    run_guarded(body("test_gemm_gpu", "test_linear_autograd_vs_fp64", shape, relu, skip), "gemm", False)


# ----------------------------------------------------------------------------------------------
# convolution
# ----------------------------------------------------------------------------------------------
def _conv():
    return importlib.import_module("test_conv_gpu")


@pytest.mark.parametrize("setting", ["fp32", "bf16", "fp32_lp"])
@pytest.mark.parametrize("shape", ["k3", "k1_to24", "k1_to96", "stem", "dil24", "direct"])
def test_conv_plan_launches(shape, setting):
    """test_conv_queries_agree_with_launches' raw-ABI sequence: its exact-size workspaces, its
    statistics buffer and its outputs are arenas, so the bytes after each are watched."""
    tc = _conv()
    assert shape in tc.PLAN_SHAPES and setting in tc.PLAN_SETTINGS
    assert len(tc.PLAN_SHAPES) == 6 and len(tc.PLAN_SETTINGS) == 3  # every entry is covered here

    def fn():
        out = tc.plan_launches(shape, setting)
        tc.check_plan_launches(shape, setting, out)
        return {k: out[k] for k in ("y", "dx", "dw", "stats", "pair")}

    run_guarded(fn, "conv")


def _odd(case):
    return any(v % 2 for v in case[2:4])


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4], ids=["auto", "gemm1", "gemm2", "gemm2_128", "gemm1x1"])
@pytest.mark.parametrize("idx", [i for i, c in enumerate(_conv().CASES) if _odd(c)])
def test_conv2d_odd_sizes(idx, variant):
    run_guarded(body("test_conv_gpu", "test_conv_fwd_bwd_vs_fp64", _conv().CASES[idx], variant,
                     settings=[raw("e2ep_conv_gemm_variant", variant)]), "conv", False)


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4], ids=["auto", "gemm1", "gemm2", "gemm2_128", "gemm1x1"])
@pytest.mark.parametrize("idx", [i for i, c in enumerate(_conv().SKIP_CASES) if c[1] % 2])
def test_conv2d_skip_odd_channels(idx, variant):
    """SKIP_CASES has no odd map; its odd member is Cin = 65 with grad_channels = 64."""
    run_guarded(body("test_conv_gpu", "test_conv_skip_gradient_fused", _conv().SKIP_CASES[idx], variant,
                     settings=[raw("e2ep_conv_gemm_variant", variant)]), "conv", False)


# ----------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ragged", "tiny_cross", "dec_self"])
def test_attention_module_p0(case):
    run_guarded(body("test_attention_gpu", "test_mha_matches_module", case), "attention", False)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("case", ["ragged", "tiny_cross", "dec_self"])
def test_attention_fused_named_cases(case, p):
    """e2ep_attn_keep_mask, the fused forward and the backward at the named shapes (ragged 77 x
    130, tiny_cross 5 x 9, dec_self 14 x 14 causal with key padding; E = 258, 6 heads of 43, B = 4)
    with dropout 0 and 0.1, against the fp64 restatement with the kernel's own keep mask: the
    reference and the 1e-4 bounds of test_attention_dropout_matches_masked_reference."""
    from e2ep_amd import _lib, attention
    ta = importlib.import_module("test_attention_gpu")
    Sq, Sk = {"ragged": (77, 130), "tiny_cross": (5, 9), "dec_self": (14, 14)}[case]
    causal = case == "dec_self"
    H, B, dh = ta.H, 4, 43
    Ed = H * dh
    g = _g(11 + Sq)
    qb = torch.randn(Sq, B, Ed, generator=g)
    kvb = torch.randn(Sk, B, 2 * Ed, generator=g)
    do = torch.randn(Sq, B, Ed, generator=g)
    kpm = torch.zeros(B, Sk, dtype=torch.bool)
    kpm[1, Sk - 3:] = True

    def heads(t):  # (S, B, H*dh) -> (B*H, S, dh)
        return t.reshape(t.shape[0], B, H, dh).permute(1, 2, 0, 3).reshape(B * H, t.shape[0], dh)

    def fn():
        seed = _put(torch.tensor([12345], dtype=torch.int32))
        keep = torch.empty(B * H, Sq, Sk, dtype=torch.uint8, device=DEV)
        _lib.call("e2ep_attn_keep_mask", _lib.ptr(seed), B * H, Sq, Sk, p, _lib.ptr(keep), _lib.stream())
        k64 = keep.cpu().double()
        assert bool((k64 == 1).all()) if p == 0 else 0.8 < float(k64.mean()) < 0.97
        qd, kvd = _put(qb, True), _put(kvb, True)
        o = attention.attention(qd, kvd, H, causal, _put(kpm), p, seed if p > 0 else None)
        (o * _put(do)).sum().backward()
        qr, kvr = qb.double().requires_grad_(True), kvb.double().requires_grad_(True)
        orr = ta._ref_core(heads(qr), heads(kvr[..., :Ed]), heads(kvr[..., Ed:]), k64, p, causal, kpm)
        orr = orr.reshape(B, H, Sq, dh).permute(2, 0, 1, 3).reshape(Sq, B, Ed)
        (orr * do.double()).sum().backward()
        assert rel_l2(o, orr) < 1e-4 and rel_l2(qd.grad, qr.grad) < 1e-4 and rel_l2(kvd.grad, kvr.grad) < 1e-4
        return {"keep": keep, "out": o, "dq": qd.grad, "dkv": kvd.grad}

    run_guarded(fn, "attention")


@pytest.mark.parametrize("Sq,Sk,causal", [(14, 14, True), (17, 9, False)])
def test_attention_dropout_and_keep_mask(Sq, Sk, causal):
    run_guarded(body("test_attention_gpu", "test_attention_dropout_matches_masked_reference", Sq, Sk, causal),
                "attention", False)


@pytest.mark.parametrize("average", [False, True], ids=["per_head", "averaged"])
@pytest.mark.parametrize("case", ["ragged", "tiny_cross", "dec_self"])
def test_attention_weights(case, average):
    run_guarded(body("test_attention_weights_gpu", "test_module_matches_stock_fp64", case, average, [],
                     comparers=("_check",)), "attention", False)


@pytest.mark.parametrize("packed,causal,p", [(True, False, 0.1), (False, False, 0.0), (True, True, 0.1)])
def test_attention_split_backward(packed, causal, p):
    run_guarded(body("test_attention_gpu", "test_split_backward_equals_serial", packed, causal, p),
                "attention", False)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_matrix_core(p):
    run_guarded(body("test_attention_gpu", "test_attention_matrix_core_matches_reference", 128, 128, p),
                "attention", False)


# ----------------------------------------------------------------------------------------------
# tokens
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 40, 66), (1, 30, 33, 31)])
def test_fusion_tokens(shape):
    run_guarded(body("test_tokens_gpu", "test_fusion_tokens_match_torch", shape), "tokens", False)


def test_embed_tokens():
    run_guarded(body("test_tokens_gpu", "test_embed_tokens_match_torch"), "tokens", False)


def test_tokens_init_and_argmax_append():
    run_guarded(body("test_tokens_gpu", "test_token_argmax_append_matches_softmax_argmax", 3, 7), "tokens", False)


# ----------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [7, 65])
def test_control_ce(V):
    """V = 7 / 65 (the suite runs 204 only): fp64 cross entropy with the PAD class ignored,
    bounds of test_control_ce_matches_reference (loss 1e-6 relative, gradient 1e-6)."""
    from e2ep_amd import losses
    B, pad = 5, V - 1
    g = _g(V)
    pred = torch.randn(B, 14, V, generator=g) * 3
    gt = torch.randint(0, V - 1, (B, 15), generator=g)
    gt[0, 9:] = pad
    gt[B - 1, 5:] = pad
    r = pred.double().requires_grad_()
    ref = F.cross_entropy(r.reshape(-1, V), gt[:, 1:].reshape(-1), ignore_index=pad)
    ref.backward()

    def fn():
        x = _put(pred, True)
        out = losses.control_ce(x, _put(gt), pad)
        out.backward()
        assert abs(float(out) / float(ref) - 1) < 1e-6 and rel_l2(x.grad, r.grad) < 1e-6
        return {"loss": out, "dx": x.grad}

    run_guarded(fn, "losses")


@pytest.mark.parametrize("hw", [(15, 17), (1, 257)])
def test_seg_weighted_ce(hw):
    """Non-square maps; fp64 weighted cross entropy (ignored pixels count in the mean), bounds
    of test_seg_weighted_ce_matches_reference."""
    from e2ep_amd import losses
    B, (h, w) = 3, hw
    g = _g(h * w + B)
    pred = torch.randn(B, 1, 3, h, w, generator=g) * 2
    tgt = torch.randint(0, 3, (B, 1, h, w), generator=g)
    tgt[0, 0, :1, :7] = 255
    wts = torch.tensor([1.0, 2.0, 2.0])
    r = pred.double().requires_grad_()
    ref = F.cross_entropy(r.view(B, 3, h, w), tgt.view(B, h, w), reduction="none", ignore_index=255,
                          weight=wts.double()).mean()
    ref.backward()

    def fn():
        x = _put(pred, True)
        out = losses.seg_weighted_ce(x, _put(tgt), wts)
        out.backward()
        assert abs(float(out) / float(ref) - 1) < 1e-6 and rel_l2(x.grad, r.grad) < 1e-6
        assert float(x.grad[0, 0, :, :1, :7].abs().max()) == 0.0
        return {"loss": out, "dx": x.grad}

    run_guarded(fn, "losses")


def test_depth_bce_smallest():
    run_guarded(body("test_losses_gpu", "test_depth_bce_matches_reference", 2, 4, 256), "losses", False)


# ----------------------------------------------------------------------------------------------
# incremental decoder
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,Sk,B,L", [("odd", 5, 3, 3), ("odd", 131, 5, 2), ("small", 5, 1, 3)])
def test_incremental_decoder(name, Sk, B, L):
    """test_ar_decode_gpu._check_steps with the (cached) module's parameters moved into guarded
    storage for the pass; the K/V caches and every step's buffers are arenas."""
    ar = importlib.import_module("test_ar_decode_gpu")
    cp, _ = ar._module(name)
    inner = body("test_ar_decode_gpu", "_check_steps", name, Sk, B, L)

    def fn():
        held = [(p, p.data) for p in list(cp.parameters()) + list(cp.buffers())]
        try:
            if guard.active() is not None:
                for p, d in held:
                    p.data = guard.put(d)
            return inner()
        finally:
            for p, d in held:
                p.data = d

    run_guarded(fn, "incremental_decoder", False)


# ----------------------------------------------------------------------------------------------
# the direct stem kernels (7x7 stride 2)
# ----------------------------------------------------------------------------------------------
def _stem():
    return importlib.import_module("test_conv_stem_gpu")


@pytest.mark.parametrize("case", _stem().CASES, ids=_ids(_stem().CASES))
def test_stem_forward_bf16(case):
    run_guarded(body("test_conv_stem_gpu", "test_stem_direct_vs_rounded_fp64", case, "bf16", torch.bfloat16),
                "conv_stem", False)


@pytest.mark.parametrize("case", _stem().DG_CASES, ids=_ids(_stem().DG_CASES))
def test_stem_dgrad_bf16(case):
    run_guarded(body("test_conv_stem_gpu", "test_stem_direct_dgrad_vs_rounded_fp64", case, "bf16",
                     torch.bfloat16), "conv_stem", False)


@pytest.mark.parametrize("case", _stem().WG_CASES, ids=_ids(_stem().WG_CASES))
def test_stem_wgrad(case):
    run_guarded(body("test_conv_stem_gpu", "test_stem_direct_wgrad_vs_rounded_fp64", case), "conv_stem", False)
    run_guarded(body("test_conv_stem_gpu", "test_stem_direct_wgrad_fp32_vs_fp64", case), "conv_stem", False)


@pytest.mark.parametrize("case", _stem().F32_CASES, ids=_ids(_stem().F32_CASES))
def test_stem_fp32(case):
    run_guarded(body("test_conv_stem_gpu", "test_stem_direct_fp32_vs_fp64", case), "conv_stem", False)


# ----------------------------------------------------------------------------------------------
# lift-splat, transposes, target plane
# ----------------------------------------------------------------------------------------------
def test_lift_splat_golden():
    """Plan (its workspace and tables), forward and backward on the lss_c4 golden geometry;
    e2ep_transpose runs inside both passes."""
    run_guarded(body("test_lss_gpu", "test_lss_fwd_bwd_matches_reference_golden"), "lift_splat", False)


def test_transpose_multi():
    run_guarded(body("test_conv_gpu", "test_tap_major_batch_one_launch_matches_per_weight"), "lift_splat", False)


def test_transpose_strided_batches():
    """lss.transpose of a (batch, rows, cols) view with a batch stride larger than rows x cols
    (the backward's gradient slice): exact data movement."""
    from e2ep_amd import lss
    x = torch.randn(3, 7 + 2, 45, generator=_g(9))

    def fn():
        xd = _put(x)
        out = lss.transpose(xd, 7, 45, 3, in_bstride=9 * 45)
        assert torch.equal(out.cpu(), x[:, :7].transpose(1, 2))
        return out

    run_guarded(fn, "lift_splat")


@pytest.mark.parametrize("xy", [(1.23, -2.71), (-10.4, -10.45), (15.0, -15.0)])
def test_target_bev(xy):
    """As test_target_bev_matches_reference_semantics: the plane is written, the other channels of
    the (exact-size) tensor are not."""
    from e2ep_amd import lss
    from oracle import parking_ref as O
    B = 3
    tp = torch.tensor([[xy[0], xy[1], 30.0]] * B)
    noise = torch.tensor([[0.0, 0.999], [0.5, 0.05], [0.93, 0.41]])
    m = O.ParkingModelRef.__new__(O.ParkingModelRef)
    m.cfg = O.Cfg
    _, ref = O.ParkingModelRef.add_target_bev(m, torch.zeros(B, 2, 200, 200), tp, noise)

    def fn():
        out = torch.full((B, 3, 200, 200), 7.0, device=DEV)
        lss.target_bev(out, 2, tp, noise, 0.1, 0.1)
        assert torch.equal(out[:, 2:].cpu(), ref) and bool((out[:, :2] == 7.0).all())
        return out

    run_guarded(fn, "lift_splat")


# ----------------------------------------------------------------------------------------------
# FlatAdam
# ----------------------------------------------------------------------------------------------
ADAM_NUMELS = [1, 3, 5, 1027, 4096 + 1]


@pytest.mark.parametrize("path", ["step", "clipped", "gather", "accumulate"])
def test_flat_adam(path):
    """Two optimizer steps over parameters of 1, 3, 5, 1027 and 4097 elements; the flat parameter,
    moment and gradient buffers, the norm partials and the device scalars are arenas.  Against the
    fp64 torch.optim.Adam chain (clip_grad_norm_ for the clipped path, the mean of two micro
    gradients for gather / accumulate), bound 1e-6 as test_optim_gpu / test_grad_clip_gpu.  The
    clipped path runs e2ep_grad_sqnorm and the finalisation."""
    from e2ep_amd.optim import FlatAdam
    g = _g(31)
    p0 = [torch.randn(n, generator=g) for n in ADAM_NUMELS]
    grads = [[[torch.randn(n, generator=g) for n in ADAM_NUMELS] for _ in range(2)] for _ in range(2)]
    micro = path in ("gather", "accumulate")
    max_norm = 0.5 if path == "clipped" else None
    ref = [p.double().requires_grad_() for p in p0]
    topt = torch.optim.Adam(ref, lr=1e-3, weight_decay=1e-4, foreach=False)
    norms = []
    for step in grads:
        for p, a, b in zip(ref, *step):
            p.grad = (a.double() + b.double()) / 2 if micro else a.double()
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ref, max_norm, foreach=False)))
        topt.step()

    def fn():
        ps = [_put(p, True) for p in p0]
        opt = FlatAdam(ps, lr=1e-3, weight_decay=1e-4, max_grad_norm=max_norm)
        flat = torch.empty(opt.numel, device=DEV) if micro else None
        has = torch.zeros(len(ps), dtype=torch.int64, device=DEV)
        out = {}
        for k, step in enumerate(grads):
            if not micro:
                for p, a in zip(ps, step[0]):
                    p.grad = _put(a)
                opt.step()
            elif path == "gather":
                for p, a, b in zip(ps, *step):
                    p.grad = _put(a + b)
                opt.prepare()
                opt.gather_grads(flat)
                opt.step(flat, 0.5)
            else:
                for i, gs in enumerate(step):
                    for p, a in zip(ps, gs):
                        p.grad = _put(a)
                    opt.prepare()
                    opt.accumulate_grads(flat, i == 0)
                    opt.has_grad(has, union=i > 0)
                opt.step(flat, 0.5, has_grad=has)
            if max_norm is not None:
                out[f"norm{k}"] = torch.empty_like(opt.grad_norm_dev).copy_(opt.grad_norm_dev)
                assert abs(float(opt.grad_norm_dev) / norms[k] - 1) < 1e-6
        for q, r in zip(ps, ref):
            assert rel_l2(q.detach(), r.detach()) < 1e-6
        out.update(flat=opt.flat, exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq, steps=opt.step_count,
                   stepped=opt.stepped, partials=opt._partials, coef=opt.clip_coef_dev)
        if micro:  # the alignment padding between two tensors' spans is never written nor read
            out["grad_flat"] = [flat[o:o + n] for o, n in opt.spans]
        return out

    run_guarded(fn, "flat_adam")


# ----------------------------------------------------------------------------------------------
# deferred parameter gradients
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [1, 2, 3])
def test_deferred_parameter_gradients(key):
    """One scope holding conv slab sums (an n that is no multiple of 64, one block, a 3x3 with a
    paired backward), a LayerNorm dgamma / dbeta record and SE weight-gradient records, with
    e2ep_tune key 37 = 1 (immediate), 2 (batched) and 3 (conv slabs only): bitwise the immediate
    results, workspaces kept alive until the flush."""
    from e2ep_amd import defer, nn_ops
    td = importlib.import_module("test_defer_pgrad_gpu")
    cases = [td.ODD, td.TINY, td.FOLD[2]]
    g = _g(37)
    rows, E, N, C, sq = 112, 258, 2, 24, 6
    host = dict(a=torch.randn(rows, E, generator=g), b=torch.randn(rows, E, generator=g),
                dy=torch.randn(rows, E, generator=g), gamma=torch.randn(E, generator=g),
                x=torch.randn(N, C, 4, 4, generator=g), dx=torch.randn(N, C, 4, 4, generator=g),
                w1=torch.randn(sq, C, 1, 1, generator=g) / C ** 0.5, b1=torch.randn(sq, generator=g),
                w2=torch.randn(C, sq, 1, 1, generator=g) / sq ** 0.5, b2=torch.randn(C, generator=g))

    def fn():
        data = [td._inputs(c) for c in cases]
        d = {k: _put(v) for k, v in host.items()}
        norm = torch.nn.LayerNorm(E).to(DEV)
        with torch.no_grad():
            norm.weight.copy_(d["gamma"])
        se = [d[k].requires_grad_(True) for k in ("w1", "b1", "w2", "b2")]
        params = [norm.weight, norm.bias] + se

        def once(scope):
            for p in params:
                p.grad = None
            with (defer.ParamGradDefer() if scope else contextlib.nullcontext()):
                out = td._run_mix(cases, data)
                nn_ops.add_drop_layer_norm(d["a"].detach().requires_grad_(True), d["b"], norm).backward(d["dy"])
                nn_ops.squeeze_excite(d["x"].detach().requires_grad_(True), *se).backward(d["dx"])
            torch.cuda.synchronize()
            return out + [p.grad for p in params]

        ref, got = once(False), once(True)
        assert len(ref) == len(got) > len(cases) + len(params)
        for i, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, b), i
        return got

    run_guarded(body_settings(fn, [tune(37, key)]), "deferred_pgrad", False)


def body_settings(fn, settings):
    def wrapped():
        with contextlib.ExitStack() as st:
            for s in settings:
                st.enter_context(s())
            return fn()
    return wrapped


# ----------------------------------------------------------------------------------------------
# frame decoding, agent pre-processing
# ----------------------------------------------------------------------------------------------
def test_decode_frames_smallest():
    """test_decode_frames_bit_exact's (3, 20) case; the decoded image and depth are returned."""
    from e2ep_amd import decode
    td = importlib.import_module("test_dataset_gpu")
    r = np.random.default_rng(60)
    rgb = r.integers(0, 256, (3, 20, 20, 3), dtype=np.uint8)
    drgb = r.integers(0, 256, (3, 20, 20, 3), dtype=np.uint8)
    drgb[0, 0, 0], drgb[-1, -1, -1] = 255, 0
    want_img, want_dep = td._cpu_decode(rgb, drgb)

    def fn():
        img, dep = decode.decode_frames(_put(torch.from_numpy(rgb)), _put(torch.from_numpy(drgb)))
        assert img.dtype == torch.float32 and dep.dtype == torch.float64
        assert torch.equal(img.cpu(), want_img) and torch.equal(dep.cpu(), want_dep)
        return img, dep

    run_guarded(fn, "decode")


def test_decode_gather_and_widen():
    run_guarded(body("test_dataset_gpu", "test_decode_gather_and_widen"), "decode", False)


@pytest.mark.parametrize("N,H,W,crop", [(1, 8, 8, 8), (2, 9, 11, 7)])
def test_decode_bgra(N, H, W, crop):
    run_guarded(body("test_agent_post_gpu", "test_decode_bgra_equals_process_image", N, H, W, crop),
                "decode", False)


@pytest.mark.parametrize("X,Y", [(7, 5), (10, 12)])
def test_slot_kernels(X, Y):
    """e2ep_slot_partials / e2ep_slot_finish over contiguous, offset, strided, channels-last and
    sliced logits; state, found flag, statistics and class image are exact-size arenas."""
    run_guarded(body("test_agent_post_gpu", "test_batched_paths_agree", X, Y, comparers=("_same",)),
                "decode", False)


# ----------------------------------------------------------------------------------------------
def test_zz_report():
    """Guarded allocations and payload bytes per family, summed over the fill A and B passes of
    the cases that ran before this one."""
    for fam, (n, nbytes) in sorted(STATS.items()):
        print(f"guarded {fam}: {n} allocations, {nbytes} payload bytes")
