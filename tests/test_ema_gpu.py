"""FlatAdam's exponential moving average of the weights (csrc/adam.hip: k_adam_ema, k_flat_swap;
e2ep_amd/optim.py) on the device.

Only the averaging arithmetic is under test where a float64 chain is the reference: after every
step the GPU's own fp32 parameters are read back and the chain e += (1 - d_t) * (p - e) is
advanced from them.  Bound 1e-6 on rel_l2 per tensor, the bound test_optim_gpu.py holds the same
kind of fp32 chain to: an update adds about three fp32 roundings (the subtraction, the fused
multiply-add, the fp32 weight) and multiplies the earlier error by d_t < 1, so over six updates
even the worst element is off by about 1e-6 relative and the L2 norm over many elements by far
less.  Everything else is compared bit for bit."""
import importlib
import os
import types

import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(5,), (64, 3, 3, 3), (4097,), (3, 7), (1, 10, 258), (20000,), (24,)]  # test_optim_gpu.py's


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(DEV).requires_grad_() for s in SHAPES]


def _grads(step, skip=()):
    g = torch.Generator().manual_seed(100 + step)
    return [None if i in skip else torch.randn(s, generator=g).to(DEV) for i, s in enumerate(SHAPES)]


def _set(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.clone()


def _host64(ps):
    return [p.detach().cpu().double() for p in ps]


def _decay(d, warmup, n):
    return min(d, (1 + n) / (10 + n)) if warmup else d


def _advance(ref, ps, d):
    for e, p in zip(ref, _host64(ps)):
        e += (1.0 - d) * (p - e)


# 1, 2 -- the arithmetic ------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("decay,warmup", [(0.5, False), (0.9, False), (0.9999, False), (0.9999, True)])
def test_ema_matches_float64_chain(decay, warmup, wd):
    from e2ep_amd.optim import FlatAdam
    ps, twin = _params(0), _params(0)
    opt = FlatAdam(ps, lr=1e-3, weight_decay=wd, ema_decay=decay, ema_warmup=warmup)
    off = FlatAdam(twin, lr=1e-3, weight_decay=wd)
    assert off.ema is None and off.ema_updates_dev is None  # off: nothing allocated
    assert torch.equal(opt.ema, opt.flat) and opt.ema.data_ptr() != opt.flat.data_ptr()
    ref = _host64(ps)
    for k in range(6):
        gs = _grads(k)
        _set(ps, gs)
        _set(twin, gs)
        opt.step()
        off.step()
        _advance(ref, ps, _decay(decay, warmup, k + 1))
        for i, e in enumerate(ref):
            err = rel_l2(opt.ema_param(i), e)
            print("ema_chain", decay, warmup, wd, k, i, f"{err:.3e}")
            assert opt.ema_param(i).shape == ps[i].shape
            assert err < 1e-6, (k, i, err)
    assert int(opt.ema_updates_dev) == 6
    if decay < 0.9999:  # the average really left the weights
        assert rel_l2(opt.ema_param(5), ps[5].detach()) > 1e-5
    # the averaging changes nothing else: a twin without it, fed the same gradients
    assert torch.equal(opt.flat, off.flat)
    assert torch.equal(opt.exp_avg, off.exp_avg) and torch.equal(opt.exp_avg_sq, off.exp_avg_sq)
    assert torch.equal(opt.step_count, off.step_count)


def test_ema_decay_range():
    from e2ep_amd.optim import FlatAdam
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            FlatAdam(_params(0), ema_decay=bad)
    FlatAdam(_params(0), ema_decay=0.0)


# 3 -- gradient sources -------------------------------------------------------------------------
def test_ema_gradient_sources_agree_bitwise():
    """Table gradients; a gathered flat buffer doubled and stepped with grad_scale 0.5 and
    has_grad (the data-parallel form); clipping with a norm bound never reached (coefficient
    exactly 1).  Step 1 leaves tensor 4 without a gradient on every path."""
    from e2ep_amd.optim import FlatAdam
    kw = dict(lr=1e-3, weight_decay=1e-4, ema_decay=0.9, ema_warmup=True)
    a, b, c = _params(2), _params(2), _params(2)
    oa, ob, oc = FlatAdam(a, **kw), FlatAdam(b, **kw), FlatAdam(c, max_grad_norm=1e9, **kw)
    flat = torch.zeros(ob.numel, device=DEV)
    has = torch.zeros(len(b), dtype=torch.int64, device=DEV)
    for k in range(3):
        gs = _grads(k, skip=(4,) if k == 1 else ())
        for ps in (a, b, c):
            _set(ps, gs)
        oa.step()
        ob.prepare()
        ob.gather_grads(flat)
        flat.mul_(2.0)  # the all-reduce sum over two ranks with the same gradient
        ob.has_grad(has)
        ob.step(flat, 0.5, has_grad=has)
        oc.step()
        assert float(oc.clip_coef_dev) == 1.0
    for o in (ob, oc):
        assert torch.equal(o.ema, oa.ema)
        assert torch.equal(o.flat, oa.flat)
        assert int(o.ema_updates_dev) == 3
    assert not torch.equal(oa.ema, oa.flat)


# 4 -- unaligned gradient -----------------------------------------------------------------------
def test_ema_unaligned_gradient_equals_aligned_bitwise():
    from e2ep_amd.optim import FlatAdam
    kw = dict(lr=1e-3, weight_decay=1e-4, ema_decay=0.9)
    a, b = _params(3), _params(3)
    oa, ob = FlatAdam(a, **kw), FlatAdam(b, **kw)
    for k in range(3):
        gs = _grads(k)
        _set(a, gs)
        _set(b, gs)
        buf = torch.zeros(gs[2].numel() + 8, device=DEV)
        b[2].grad = buf[1:1 + gs[2].numel()].copy_(gs[2])
        assert b[2].grad.data_ptr() % 16 == 4 and a[2].grad.data_ptr() % 16 == 0
        oa.step()
        ob.step()
    assert torch.equal(oa.ema, ob.ema) and torch.equal(oa.flat, ob.flat)
    assert not torch.equal(oa.ema_param(2), a[2].detach())


# 5 -- missing gradient -------------------------------------------------------------------------
def test_ema_tensor_without_gradient():
    from e2ep_amd.optim import FlatAdam
    decay = 0.9
    ps = _params(4)
    opt = FlatAdam(ps, lr=1e-2, weight_decay=1e-4, ema_decay=decay)
    init6 = ps[6].detach().clone()
    ref = _host64(ps)
    o2, n2 = opt.spans[2]
    for k, skip in enumerate([(6,), (2, 6), (6,)]):
        before = (ps[2].detach().clone(), opt.exp_avg[o2:o2 + n2].clone(),
                  opt.exp_avg_sq[o2:o2 + n2].clone())
        _set(ps, _grads(k, skip=skip))
        opt.step()
        _advance(ref, ps, decay)
        if k == 1:  # tensor 2: weights and moments untouched, the average still moves
            assert torch.equal(ps[2].detach(), before[0])
            assert torch.equal(opt.exp_avg[o2:o2 + n2], before[1])
            assert torch.equal(opt.exp_avg_sq[o2:o2 + n2], before[2])
            assert not torch.equal(opt.ema_param(2), ps[2].detach())
            err = rel_l2(opt.ema_param(2), ref[2])
            print("ema_missing", f"{err:.3e}")
            assert err < 1e-6
        else:
            assert not torch.equal(ps[2].detach(), before[0])
        # never stepped: ema == p from construction, and the update is the identity
        assert torch.equal(opt.ema_param(6), ps[6].detach())
        assert torch.equal(ps[6].detach(), init6)
    assert opt.stepped.cpu().tolist() == [1, 1, 1, 1, 1, 1, 0]
    for i, e in enumerate(ref):
        assert rel_l2(opt.ema_param(i), e) < 1e-6


# 6 -- skipped step -----------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, 1.0])
def test_ema_skipped_step_changes_nothing(clip):
    from e2ep_amd.optim import FlatAdam
    ps = _params(5)
    opt = FlatAdam(ps, lr=1e-3, weight_decay=1e-4, max_grad_norm=clip, skip_nonfinite=True,
                   ema_decay=0.9, ema_warmup=True)

    def state():
        return [t.clone() for t in (opt.ema, opt.ema_updates_dev, opt.flat, opt.exp_avg,
                                    opt.exp_avg_sq, opt.step_count, opt.stepped)]

    _set(ps, _grads(0))
    opt.step()
    s0 = state()
    assert int(opt.ema_updates_dev) == 1 and int(opt.skipped_dev) == 0
    for n, bad in enumerate((float("inf"), float("nan"))):
        gs = _grads(1 + n)
        gs[1].view(-1)[7] = bad
        _set(ps, gs)
        opt.step()
        for t0, t1 in zip(s0, state()):
            assert torch.equal(t0, t1)
        assert int(opt.skipped_dev) == n + 1
    _set(ps, _grads(3))
    opt.step()
    s1 = state()
    assert all(not torch.equal(t0, t1) for t0, t1 in zip(s0[:6], s1[:6]))
    assert int(opt.ema_updates_dev) == 2 and float(opt.step_count) == 2.0 and int(opt.skipped_dev) == 2
    assert bool(torch.isfinite(opt.ema).all()) and bool(torch.isfinite(opt.flat).all())


# 7 -- the swap ---------------------------------------------------------------------------------
def test_ema_weights_swaps_contents_in_place(monkeypatch):
    from e2ep_amd import _lib
    from e2ep_amd.optim import FlatAdam
    ps = _params(6)
    opt = FlatAdam(ps, lr=1e-2, ema_decay=0.5)
    for k in range(2):
        _set(ps, _grads(k))
        opt.step()
    live = [p.detach().clone() for p in ps]
    avg = [opt.ema_param(i).clone() for i in range(len(ps))]
    flat0, ema0 = opt.flat.clone(), opt.ema.clone()
    ptrs = [p.data_ptr() for p in ps]
    assert not any(torch.equal(x, y) for x, y in zip(live, avg))
    assert not opt.ema_active
    with opt.ema_weights() as inside:
        assert inside is opt and opt.ema_active
        for i, p in enumerate(ps):
            assert torch.equal(p.detach(), avg[i])
            assert torch.equal(opt.ema_param(i), live[i])
        assert [p.data_ptr() for p in ps] == ptrs
        assert torch.equal(opt.flat, ema0) and torch.equal(opt.ema, flat0)  # pads included
        with pytest.raises(_lib.E2EPError, match="ema_weights"):
            with opt.ema_weights():
                pass
        for call in (opt.step, opt.reset_ema, lambda: opt.load_ema_state({}),
                     lambda: opt.accumulate_grads(torch.zeros(opt.numel, device=DEV), True)):
            with pytest.raises(_lib.E2EPError, match="ema_weights"):
                call()
        assert torch.equal(opt.flat, ema0) and torch.equal(opt.ema, flat0)  # the refusals did nothing
    assert not opt.ema_active
    for i, p in enumerate(ps):
        assert torch.equal(p.detach(), live[i]) and torch.equal(opt.ema_param(i), avg[i])
    assert [p.data_ptr() for p in ps] == ptrs
    assert torch.equal(opt.flat, flat0) and torch.equal(opt.ema, ema0)
    # an exception inside the block still swaps back
    with pytest.raises(ZeroDivisionError):
        with opt.ema_weights():
            1 / 0
    assert not opt.ema_active and torch.equal(opt.flat, flat0) and torch.equal(opt.ema, ema0)
    # off: no average to swap in
    plain = FlatAdam(_params(6), lr=1e-2)
    with pytest.raises(_lib.E2EPError, match="off"):
        with plain.ema_weights():
            pass
    with pytest.raises(_lib.E2EPError, match="off"):
        plain.ema_param(0)
    # during stream capture
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(_lib.E2EPError, match="capture"):
            with opt.ema_weights():
                pass
        with pytest.raises(_lib.E2EPError, match="capture"):
            opt.reset_ema()
    assert torch.equal(opt.flat, flat0) and torch.equal(opt.ema, ema0)


# one float4 per thread up to the grid cap (2048 workgroups of 256), then the grid-stride loop
@pytest.mark.parametrize("n", [4, 4 * 257, 4 * (2048 * 256 + 257)])
def test_flat_swap_entry_point(n):
    from e2ep_amd import _lib
    g = torch.Generator().manual_seed(n)
    a0, b0 = torch.randn(n + 4, generator=g).to(DEV), torch.randn(n + 4, generator=g).to(DEV)
    a, b = a0.clone(), b0.clone()
    _lib.call("e2ep_flat_swap", _lib.ptr(a), _lib.ptr(b), n, _lib.stream())
    assert torch.equal(a[:n], b0[:n]) and torch.equal(b[:n], a0[:n])
    assert torch.equal(a[n:], a0[n:]) and torch.equal(b[n:], b0[n:])  # nothing past n
    for bad in (n - 1, n + 2, 0, -4):
        with pytest.raises(_lib.E2EPError, match="multiple of 4"):
            _lib.call("e2ep_flat_swap", _lib.ptr(a), _lib.ptr(b), bad, _lib.stream())
    with pytest.raises(_lib.E2EPError, match="same buffer"):
        _lib.call("e2ep_flat_swap", _lib.ptr(a), _lib.ptr(a), n, _lib.stream())
    if n > 4:
        with pytest.raises(_lib.E2EPError, match="overlap"):
            _lib.call("e2ep_flat_swap", _lib.ptr(a), _lib.ptr(a[4:]), n, _lib.stream())
    assert torch.equal(a[:n], b0[:n]) and torch.equal(b[:n], a0[:n])  # the refused calls did nothing


# 8 -- off is off -------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True])
def test_entry_point_calls_with_ema_off_and_on(monkeypatch, clip):
    from e2ep_amd import _lib
    from e2ep_amd.optim import FlatAdam
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if clip else {}
    off, on = _params(7), _params(7)
    o_off, o_on = FlatAdam(off, lr=1e-3, **kw), FlatAdam(on, lr=1e-3, ema_decay=0.9, **kw)
    names, orig = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return orig(name, *args)

    monkeypatch.setattr(_lib, "call", recording)
    front = ["e2ep_grad_sqnorm", "e2ep_grad_norm_finalize"] if clip else []
    _set(off, _grads(0))
    o_off.step()
    assert names == front + ["e2ep_adam_step_clipped" if clip else "e2ep_adam_step"]
    del names[:]
    _set(on, _grads(0))
    o_on.step()
    assert names == front + ["e2ep_adam_step_ema"]
    assert torch.equal(o_on.flat, o_off.flat)


# 9 -- TrainStep on an MLP ----------------------------------------------------------------------
class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.a = torch.nn.Linear(16, 32)
        self.b = torch.nn.Linear(32, 4)

    def training_step(self, batch, idx=0):
        return (self.b(self.a(batch["x"]).relu()) - batch["y"]).pow(2).mean()


def _small_batch(seed):
    g = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(8, 16, generator=g).to(DEV), "y": torch.randn(8, 4, generator=g).to(DEV)}


def _mlp_run(graph, calls, **kw):
    """Two warm-up calls on the construction batch (the graph-mode constructor makes them
    itself), then `calls` calls on alternating batches."""
    from e2ep_amd.train import TrainStep
    m = _Small().to(DEV)
    s = TrainStep(m, _small_batch(1), graph=graph, warmup=2, ema_decay=0.9, ema_warmup=True, **kw)
    if not graph:
        s(), s()
    for k in range(calls):
        s(_small_batch(2 + k % 2))
    return s


def test_train_step_captured_equals_eager():
    from e2ep_amd import _lib
    se, sg = _mlp_run(False, 5), _mlp_run(True, 5)
    assert sg.g_opt is not None and sg.opt.ema_decay == 0.9 and sg.opt.ema_warmup is True
    assert torch.equal(sg.opt.ema, se.opt.ema) and torch.equal(sg.opt.flat, se.opt.flat)
    assert int(sg.opt.ema_updates_dev) == int(se.opt.ema_updates_dev) == 2 + 5
    assert not torch.equal(sg.opt.ema, sg.opt.flat)
    for s in (se, sg):
        before = s.opt.flat.clone()
        with s.opt.ema_weights():
            with pytest.raises(_lib.E2EPError, match="ema_weights"):
                s()
            with pytest.raises(_lib.E2EPError, match="ema_weights"):
                s(_small_batch(2))
        assert torch.equal(s.opt.flat, before)
        s()  # fine again outside


def test_train_step_accumulation_moves_the_average_once_per_cycle():
    se, sg = _mlp_run(False, 6, accumulate=2), _mlp_run(True, 6, accumulate=2)
    assert torch.equal(sg.opt.ema, se.opt.ema) and torch.equal(sg.opt.flat, se.opt.flat)
    # 2 warm-up + 6 calls = 8 micro-steps = 4 updates
    assert int(sg.opt.ema_updates_dev) == int(se.opt.ema_updates_dev) == (2 + 6) // 2
    assert float(sg.opt.step_count) == 4.0


def test_train_step_ema_precedence():
    """The argument, then module.cfg, then the passed-in optimizer; enabled before the first
    (warm-up) step, so every step is counted."""
    from e2ep_amd.optim import FlatAdam
    from e2ep_amd.train import TrainStep

    def build(cfg=None, opt_kw=None, **kw):
        m = _Small().to(DEV)
        if cfg is not None:
            m.cfg = types.SimpleNamespace(**cfg)
        opt = FlatAdam(list(m.parameters()), lr=1e-4, **opt_kw) if opt_kw is not None else None
        s = TrainStep(m, _small_batch(1), graph=False, optimizer=opt, **kw)
        return s.opt

    o = build()
    assert o.ema is None and o.ema_decay is None
    o = build(cfg=dict(ema_decay=0.5, ema_warmup=True))
    assert (o.ema_decay, o.ema_warmup) == (0.5, True) and o.ema is not None
    o = build(cfg=dict(ema_decay=0.5, ema_warmup=True), ema_decay=0.25, ema_warmup=False)
    assert (o.ema_decay, o.ema_warmup) == (0.25, False)
    o = build(cfg=dict(ema_decay=None, ema_warmup=False), opt_kw=dict(ema_decay=0.75, ema_warmup=True))
    assert (o.ema_decay, o.ema_warmup) == (0.75, True)
    o = build(opt_kw={}, ema_decay=0.125)  # switched on in a passed-in optimizer
    assert (o.ema_decay, o.ema_warmup) == (0.125, False) and torch.equal(o.ema, o.flat)
    with pytest.raises(ValueError, match="ema_decay"):
        build(ema_decay=1.0)


# 10 -- captured graphs see the swap (full model) -----------------------------------------------
def _full_module(train):
    from tool.config import default_cfg
    from trainer.pl_trainer import ParkingTrainingModule
    from weights import make_state
    mod = ParkingTrainingModule(default_cfg(deterministic=True))
    mod.parking_model.load_state_dict(make_state(mod.parking_model.state_dict(), 1234))
    mod = mod.to(DEV)
    if not train:
        return mod.eval()
    for p in mod.parking_model.bev_encoder.layer4.parameters():
        p.requires_grad_(False)
    return mod.train()


def test_captured_val_step_sees_the_swap_full_model():
    from e2ep_amd import checkpoint, synthetic
    from e2ep_amd.train import TrainStep
    from e2ep_amd.val import ValStep
    d = synthetic.synthetic_batch(2, seed=7)
    data = {k: (v if k in ("intrinsics", "extrinsics") else v.to(DEV)) for k, v in d.items()}
    noise = synthetic.target_noise(2, seed=7).to(DEV)
    m = _full_module(train=True)
    m.parking_model._noise = lambda b, device, n: noise  # fixed target jitter
    step = TrainStep(m, dict(data), graph=True, warmup=1, ema_decay=0.5)
    for _ in range(3):
        step()
    opt = step.opt
    assert int(opt.ema_updates_dev) == 4
    val = ValStep(m, data, noise=noise, graph=True, warmup=1)
    assert val._graph is not None
    ptrs = [p.data_ptr() for p in opt.params]
    live = val().clone()
    with opt.ema_weights():
        averaged = val().clone()
    live2 = val().clone()
    assert [p.data_ptr() for p in opt.params] == ptrs
    ck = checkpoint.checkpoint_dict(m, opt)
    assert list(ck["ema"]["state_dict"]) == list(ck["state_dict"])
    m2 = _full_module(train=False)
    m2.load_state_dict({k: v.to(DEV) for k, v in ck["ema"]["state_dict"].items()})
    eager = ValStep(m2, data, noise=noise, graph=False)().clone()
    vals = [float(x) for x in (live, averaged, live2, eager)]
    print("val_loss live / averaged / live again / eager on the ema checkpoint:", vals)
    assert all(torch.isfinite(x) for x in (live, averaged, eager))
    assert averaged.cpu().numpy().tobytes() == eager.cpu().numpy().tobytes(), vals
    assert live.cpu().numpy().tobytes() == live2.cpu().numpy().tobytes(), vals
    assert float(averaged) != float(live), vals
    # frozen parameters and buffers in the entry are the live ones
    own = {id(p) for p in opt.params}
    names = {n: p for n, p in m.named_parameters()}
    for k, v in ck["state_dict"].items():
        if k not in names or id(names[k]) not in own:
            assert torch.equal(ck["ema"]["state_dict"][k], v), k


# 11 -- guard bands -----------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["table", "flat"])
def test_guarded_ema_step_and_swap(path):
    """test_guarded_ops_gpu.py::test_flat_adam's way: two clipped steps with the average on (step
    1 leaves the 1027-element tensor without a gradient: the average-only rows) and the swap,
    unguarded and under both fills; every flat buffer, the average and its counter are arenas."""
    G = importlib.import_module("test_guarded_ops_gpu")
    from e2ep_amd.optim import FlatAdam
    g = G._g(41)
    p0 = [torch.randn(n, generator=g) for n in G.ADAM_NUMELS]
    grads = [[torch.randn(n, generator=g) for n in G.ADAM_NUMELS] for _ in range(2)]
    grads[1][3] = None
    decay = 0.9

    def fn():
        ps = [G._put(p, True) for p in p0]
        opt = FlatAdam(ps, lr=1e-3, weight_decay=1e-4, max_grad_norm=0.5, ema_decay=decay,
                       ema_warmup=True)
        flat = torch.empty(opt.numel, device=DEV) if path == "flat" else None
        has = torch.zeros(len(ps), dtype=torch.int64, device=DEV)
        ref = [p.double() for p in p0]
        for k, step in enumerate(grads):
            for p, a in zip(ps, step):
                p.grad = None if a is None else G._put(a)
            if path == "table":
                opt.step()
            else:
                opt.prepare()
                opt.gather_grads(flat)
                opt.has_grad(has)
                opt.step(flat, 1.0, has_grad=has)
            _advance(ref, ps, _decay(decay, True, k + 1))
        for i, e in enumerate(ref):
            assert rel_l2(opt.ema_param(i), e) < 1e-6
        live, avg = opt.flat.clone(), opt.ema.clone()
        with opt.ema_weights():
            inside = opt.flat.clone()
            assert torch.equal(inside, avg) and torch.equal(opt.ema, live)
        assert torch.equal(opt.flat, live) and torch.equal(opt.ema, avg)
        return dict(flat=opt.flat, ema=opt.ema, exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq,
                    steps=opt.step_count, updates=opt.ema_updates_dev, inside=inside,
                    coef=opt.clip_coef_dev, partials=opt._partials)

    G.run_guarded(fn, "flat_adam_ema")


# -- checkpoint round trip ----------------------------------------------------------------------
class _Wrapped(torch.nn.Module):
    """A stand-in for ParkingTrainingModule: `parking_model` (with a BatchNorm, for buffers) and
    `cfg`, which is all checkpoint.py reads."""

    def __init__(self, seed):
        super().__init__()
        from tool.config import default_cfg
        torch.manual_seed(seed)
        self.parking_model = torch.nn.Sequential(torch.nn.Linear(16, 33), torch.nn.BatchNorm1d(33),
                                                 torch.nn.ReLU(), torch.nn.Linear(33, 4))
        self.cfg = default_cfg()

    def training_step(self, batch, idx=0):
        return (self.parking_model(batch["x"]) - batch["y"]).pow(2).mean()


def _train(m, opt, seeds):
    for s in seeds:
        opt.zero_grad()
        m.training_step(_small_batch(s)).backward()
        opt.step()


def test_checkpoint_round_trip_restores_the_average(tmp_path):
    from e2ep_amd import checkpoint
    from e2ep_amd.optim import FlatAdam
    m1 = _Wrapped(1).to(DEV).train()
    o1 = FlatAdam(list(m1.parameters()), lr=1e-2, weight_decay=1e-4, ema_decay=0.9, ema_warmup=True)
    _train(m1, o1, (1, 2, 3))
    path = os.path.join(tmp_path, "ema.ckpt")
    checkpoint.save_checkpoint(path, m1, o1, epoch=1, global_step=3)
    ck = checkpoint.load_checkpoint(path)  # weights_only
    e = ck["ema"]
    assert (e["decay"], e["warmup"], e["num_updates"]) == (0.9, True, 3)
    assert list(e["state_dict"]) == list(ck["state_dict"])
    params = dict(m1.named_parameters())
    for i, p in enumerate(o1.params):
        name = next(n for n, q in params.items() if q is p)
        assert torch.equal(e["state_dict"][name], o1.ema_param(i).cpu())
        assert not torch.equal(e["state_dict"][name], ck["state_dict"][name])
    for k in ck["state_dict"]:
        if k not in params:  # BatchNorm's running statistics: the live ones
            assert torch.equal(e["state_dict"][k], ck["state_dict"][k])
    torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in o1.params]).load_state_dict(
        ck["optimizer_states"][0])  # still torch.optim.Adam's format
    assert "ema" not in ck["optimizer_states"][0]
    # resume into a fresh module and an optimizer with other averaging settings
    m2 = _Wrapped(2).to(DEV).train()
    o2 = FlatAdam(list(m2.parameters()), lr=1e-2, weight_decay=1e-4, ema_decay=0.5)
    checkpoint.restore_training(ck, m2, o2)
    assert torch.equal(o2.ema, o1.ema) and torch.equal(o2.flat, o1.flat)
    assert torch.equal(o2.ema_updates_dev, o1.ema_updates_dev)
    assert (o2.ema_decay, o2.ema_warmup) == (0.9, True)
    st = o2.ema_state()
    assert (st["decay"], st["warmup"], st["num_updates"]) == (0.9, True, 3)
    assert torch.equal(st["flat"], o1.ema) and st["flat"].data_ptr() != o2.ema.data_ptr()
    _train(m1, o1, (4,))
    _train(m2, o2, (4,))
    assert torch.equal(o2.flat, o1.flat) and torch.equal(o2.ema, o1.ema)
    assert int(o2.ema_updates_dev) == 4
    # a checkpoint without the entry: the average restarts at the loaded weights
    plain = {k: v for k, v in ck.items() if k != "ema"}
    m3 = _Wrapped(3).to(DEV).train()
    o3 = FlatAdam(list(m3.parameters()), lr=1e-2, weight_decay=1e-4, ema_decay=0.9)
    _train(m3, o3, (5,))
    assert not torch.equal(o3.ema, o3.flat) and int(o3.ema_updates_dev) == 1
    checkpoint.restore_training(plain, m3, o3)
    assert torch.equal(o3.ema, o3.flat) and int(o3.ema_updates_dev) == 0
    for i, p in enumerate(o3.params):
        assert torch.equal(p.detach().cpu(), ck["state_dict"][next(n for n, q in m3.named_parameters() if q is p)])
        assert torch.equal(o3.ema_param(i), p.detach())
