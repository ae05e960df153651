"""Gradient-norm clipping, skipping of non-finite updates and gradient accumulation in FlatAdam
(csrc/adam.hip: k_gnorm_partial, k_gnorm_final, k_adam_clip, k_grad_accum) and TrainStep.

Reference for numbers: torch's own chain in fp64 on the CPU — parameters and gradients cast to
double, torch.nn.utils.clip_grad_norm_, torch.optim.Adam(foreach=False).  torch's fp32 chain is
within 9.9e-8 rel-L2 of it on the tensor set below (5.5e-8 with three accumulated
micro-gradients) and adam.hip repeats torch's fp32 operation order with contraction off, so the
parameter bound is the 1e-6 of test_optim_gpu.py.  The norm is held to the error of torch's
own fp32 clip_grad_norm_ on the device in the same test, or 1.2e-7 (one fp32 ulp), whichever
is larger; the kernel sums in fp64, so it sits at fp64 rounding.
"""
import os
import socket

import pytest
import torch
import torch.distributed as dist

from helpers import rel_l2
from test_optim_gpu import SHAPES, _grads, _params

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 1.2e-7


def _ref_chain(seed, grad_sets, max_norm, wd, lr=1e-3):
    """The fp64 CPU chain over grad_sets (lists of device tensors or None).  Returns the
    parameters, the optimizer and the norm clip_grad_norm_ returned at every step."""
    ref = [p.detach().cpu().double().requires_grad_() for p in _params(seed)]
    topt = torch.optim.Adam(ref, lr=lr, weight_decay=wd, foreach=False)
    norms = []
    for gs in grad_sets:
        for p, g in zip(ref, gs):
            p.grad = None if g is None else g.detach().cpu().double()
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(
                [p for p in ref if p.grad is not None], max_norm, foreach=False)))
        topt.step()
    return ref, topt, norms


def _torch_fp32_norm(gs, max_norm):
    """What torch's fp32 clip_grad_norm_ returns for these gradients on the device."""
    ps = [torch.zeros_like(g).requires_grad_() for g in gs if g is not None]
    for p, g in zip(ps, [g for g in gs if g is not None]):
        p.grad = g.clone()
    return float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False).double())


def _set(params, gs):
    for p, g in zip(params, gs):
        p.grad = None if g is None else g.clone()


def _norm_bound(want, gs, max_norm):
    return max(abs(_torch_fp32_norm(gs, max_norm) - want) / want, ULP)


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa["state"]) == sorted(sb["state"]) and sa["param_groups"] == sb["param_groups"]
    for i in sa["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa["state"][i][k], sb["state"][i][k]), (i, k)


# 1 -- clipped steps against the fp64 chain -----------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("max_norm", [1.0, 50.0, 1e9])
def test_clipped_steps_match_fp64_chain(max_norm, wd):
    from e2ep_amd.optim import FlatAdam
    sets = [_grads(k) for k in range(6)]
    ref, _, norms = _ref_chain(0, sets, max_norm, wd)
    mine = _params(0)
    opt = FlatAdam(mine, lr=1e-3, weight_decay=wd, max_grad_norm=max_norm)
    for gs, want in zip(sets, norms):
        _set(mine, gs)
        opt.step()
        got = float(opt.grad_norm_dev)
        bound = _norm_bound(want, gs, max_norm)
        print(f"norm {got!r} fp64 {want!r} rel {abs(got - want) / want:.3e} bound {bound:.3e}")
        assert abs(got - want) / want <= bound
        coef = float(opt.clip_coef_dev)
        assert (coef < 1.0) == (max_norm < 169.0) and 160.0 < want < 180.0
        assert abs(coef - min(max_norm / (want + 1e-6), 1.0)) <= ULP * coef
    for p, q in zip(ref, mine):
        err = rel_l2(q.detach(), p.detach())
        print(f"param rel-L2 {err:.3e}")
        assert err < 1e-6
    assert int(opt.skipped_dev) == 0


def test_more_rows_than_the_finalisation_has_threads():
    """A 1025-row tensor (plus three elements: an odd tail) on top of the usual set: the
    finalisation's 256 threads each add several partials.  One clipped step."""
    from e2ep_amd import _lib
    from e2ep_amd.optim import FlatAdam
    n = 1025 * _lib.load().e2ep_adam_chunk_elems() + 3
    g = torch.Generator().manual_seed(77)
    big_p, big_g = torch.randn(n, generator=g), torch.randn(n, generator=g)
    gs = _grads(0) + [big_g.to(DEV)]
    ref = [p.detach().cpu().double().requires_grad_() for p in _params(0)] + \
        [big_p.double().requires_grad_()]
    for p, x in zip(ref, gs):
        p.grad = x.cpu().double()
    want = float(torch.nn.utils.clip_grad_norm_(ref, 1.0, foreach=False))
    torch.optim.Adam(ref, lr=1e-3, weight_decay=1e-4, foreach=False).step()
    mine = _params(0) + [big_p.to(DEV).requires_grad_()]
    opt = FlatAdam(mine, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    assert opt.n_chunks > 1025 + len(SHAPES)
    _set(mine, gs)
    opt.step()
    got = float(opt.grad_norm_dev)
    assert abs(got - want) / want <= _norm_bound(want, gs, 1.0)
    for p, q in zip(ref, mine):
        assert rel_l2(q.detach(), p.detach()) < 1e-6


# 2 -- coefficient 1 is the identity ------------------------------------------------------------
@pytest.mark.parametrize("path", ["table", "flat"])
def test_coefficient_one_is_the_identity(path):
    from e2ep_amd.optim import FlatAdam
    a, b = _params(2), _params(2)
    oa = FlatAdam(a, lr=1e-3, weight_decay=1e-4)
    ob = FlatAdam(b, lr=1e-3, weight_decay=1e-4, max_grad_norm=1e9)
    fa, fb = torch.zeros(oa.numel, device=DEV), torch.zeros(ob.numel, device=DEV)
    for k in range(3):
        gs = _grads(k, skip=3 if k == 1 else None)
        for o, ps, f in ((oa, a, fa), (ob, b, fb)):
            _set(ps, gs)
            if path == "table":
                o.step()
            else:
                o.prepare()
                o.gather_grads(f)
                f.mul_(2.0)
                o.step(f, 0.5)
        assert float(ob.clip_coef_dev) == 1.0
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())
    assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
    _same_state(oa, ob)


# 3 -- reproducible -----------------------------------------------------------------------------
def _norm_bits(opt):
    return opt.grad_norm_dev.clone().view(torch.int64).item()


def test_norm_is_reproducible_bitwise():
    from e2ep_amd import graphs
    from e2ep_amd.optim import FlatAdam
    gs = _grads(0)
    bits = []
    # two table runs; the 4097-element gradient as an unaligned view (k_adam's scalar path)
    for unaligned in (False, False, True):
        ps = _params(3)
        opt = FlatAdam(ps, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
        _set(ps, gs)
        if unaligned:
            buf = torch.zeros(gs[2].numel() + 8, device=DEV)
            ps[2].grad = buf[1:1 + gs[2].numel()].copy_(gs[2])
            assert ps[2].grad.data_ptr() % 16 == 4
        opt.step()
        bits.append(_norm_bits(opt))
        keep = [p.detach().clone() for p in ps]
    # the same gradients gathered into a flat buffer
    ps = _params(3)
    opt = FlatAdam(ps, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    flat = torch.zeros(opt.numel, device=DEV)
    _set(ps, gs)
    opt.prepare()
    opt.gather_grads(flat)
    opt.step(flat, 1.0)
    bits.append(_norm_bits(opt))
    for p, q in zip(keep, ps):
        assert torch.equal(p, q.detach())  # and so is the clipped update
    # a captured replay of the table step
    ps = _params(3)
    opt = FlatAdam(ps, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    _set(ps, gs)
    opt.prepare()
    torch.cuda.synchronize()
    g, _, _ = graphs.capture(opt.step)
    assert float(opt.grad_norm_dev) == 0.0  # the capture itself ran nothing
    g.replay()
    bits.append(_norm_bits(opt))
    for p, q in zip(keep, ps):
        assert torch.equal(p, q.detach())
    assert len(set(bits)) == 1, bits


# 4 -- missing gradient -------------------------------------------------------------------------
def test_missing_gradient_is_left_out_of_norm_and_step():
    from e2ep_amd.optim import FlatAdam
    gs = _grads(0, skip=2)
    ref, topt, norms = _ref_chain(1, [gs], 1.0, 0.0, lr=1e-2)
    ps = _params(1)
    before = ps[2].detach().clone()
    opt = FlatAdam(ps, lr=1e-2, max_grad_norm=1.0)
    _set(ps, gs)
    opt.step()
    got, want = float(opt.grad_norm_dev), norms[0]
    assert abs(got - want) / want <= _norm_bound(want, gs, 1.0)
    assert torch.equal(ps[2].detach(), before)
    assert sorted(opt.state_dict()["state"]) == sorted(topt.state_dict()["state"]) == [
        i for i in range(len(SHAPES)) if i != 2]
    for i, (p, q) in enumerate(zip(ref, ps)):
        assert rel_l2(q.detach(), p.detach()) < 1e-6, i


# 5 -- value edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [1e30, 1e-30, 0.0])
def test_value_edges(fill):
    """1e30: an fp32 sum of squares overflows, the fp64 one gives a finite norm and the clipped
    step follows the fp64 chain.  1e-30: the squares vanish in fp32, not in fp64.  0: norm 0,
    coefficient exactly 1 (1 / 1e-6 limited to 1), nothing moves (no weight decay)."""
    from e2ep_amd.optim import FlatAdam
    gs = [torch.full(s, fill, device=DEV) for s in SHAPES]
    ref, _, norms = _ref_chain(4, [gs], 1.0, 0.0)
    ps = _params(4)
    before = [p.detach().clone() for p in ps]
    opt = FlatAdam(ps, lr=1e-3, max_grad_norm=1.0)
    _set(ps, gs)
    opt.step()
    got, want = float(opt.grad_norm_dev), norms[0]
    if fill == 0.0:
        assert got == 0.0 and want == 0.0 and float(opt.clip_coef_dev) == 1.0
        for p, b in zip(ps, before):
            assert torch.equal(p.detach(), b)
        return
    n = sum(p.numel() for p in ps)
    exact = float(torch.tensor(fill, dtype=torch.float32).double()) * n ** 0.5
    assert got > 0.0 and got != float("inf")
    assert abs(got - want) / want <= ULP and abs(got - exact) / exact <= ULP
    for p, q in zip(ref, ps):
        assert rel_l2(q.detach(), p.detach()) < 1e-6


# 6 -- non-finite gradients ---------------------------------------------------------------------
def _bad(bad):
    """A finite gradient set with `bad` in the last element of the last row of the 4097-element
    tensor (row 2 of that tensor holds this one element: a tail a vector-load guard can drop)."""
    gs = _grads(9)
    gs[2][4096] = bad
    return gs


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_skip_nonfinite_leaves_everything_unchanged(bad):
    from e2ep_amd.optim import FlatAdam
    a, b = _params(5), _params(5)
    oa = FlatAdam(a, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    ob = FlatAdam(b, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    start = oa.flat.clone()
    # a bad first step: nothing is stepped, no tensor gets state
    _set(a, _bad(bad))
    oa.step()
    assert int(oa.skipped_dev) == 1 and not torch.isfinite(oa.grad_norm_dev).item()
    assert torch.equal(oa.flat, start) and float(oa.step_count) == 0.0
    assert not oa.exp_avg.any() and not oa.exp_avg_sq.any() and not oa.stepped.any()
    assert oa.state_dict()["state"] == {}
    for k in range(3):
        for o, ps in ((oa, a), (ob, b)):
            _set(ps, _grads(k))
            o.step()
        if k == 0:  # a bad step in the middle: bitwise unchanged
            snap = (oa.flat.clone(), oa.exp_avg.clone(), oa.exp_avg_sq.clone(),
                    oa.step_count.clone(), oa.stepped.clone())
            _set(a, _bad(bad))
            oa.step()
            now = (oa.flat, oa.exp_avg, oa.exp_avg_sq, oa.step_count, oa.stepped)
            assert all(torch.equal(x, y) for x, y in zip(snap, now))
            assert int(oa.skipped_dev) == 2
    # the run that never saw the bad steps
    assert int(ob.skipped_dev) == 0 and float(oa.step_count) == float(ob.step_count) == 3.0
    assert torch.equal(oa.flat, ob.flat)
    assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
    _same_state(oa, ob)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_without_skip_follows_the_torch_chain(bad):
    """skip_nonfinite=False with a max_grad_norm: what torch's chain gives.  A NaN makes the norm
    and the coefficient NaN (torch.clamp lets it through; an fmin-style limit would make it 1),
    so every value of every stepped parameter is NaN.  An Inf makes the norm Inf and the
    coefficient 0: Inf * 0 = NaN in that one element, 0 everywhere else — the torch chain's NaN
    pattern is the reference, and the finite values agree with it."""
    from e2ep_amd.optim import FlatAdam
    gs = _bad(bad)
    ref, _, _ = _ref_chain(5, [gs], 1.0, 0.0)
    ps = _params(5)
    opt = FlatAdam(ps, lr=1e-3, max_grad_norm=1.0)
    _set(ps, gs)
    opt.step()
    assert int(opt.skipped_dev) == 0 and float(opt.step_count) == 1.0
    coef = float(opt.clip_coef_dev)
    assert coef != coef if bad != bad else coef == 0.0
    for i, (p, q) in enumerate(zip(ref, ps)):
        pn, qn = p.detach().isnan(), q.detach().cpu().isnan()
        assert torch.equal(pn, qn), i
        if bad != bad:
            assert qn.all(), i
        else:
            assert int(qn.sum()) == (1 if i == 2 else 0)
            assert rel_l2(q.detach().cpu()[~qn], p.detach()[~pn]) < 1e-6


def test_skip_without_clipping_keeps_coefficient_one():
    from e2ep_amd.optim import FlatAdam
    a, b = _params(6), _params(6)
    oa, ob = FlatAdam(a, lr=1e-3), FlatAdam(b, lr=1e-3, skip_nonfinite=True)
    for k in range(2):
        for o, ps in ((oa, a), (ob, b)):
            _set(ps, _grads(k))
            o.step()
        assert float(ob.clip_coef_dev) == 1.0 and float(ob.grad_norm_dev) > 100.0
    assert torch.equal(oa.flat, ob.flat) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
    _set(b, _bad(float("nan")))
    ob.step()
    assert float(ob.clip_coef_dev) == 1.0 and int(ob.skipped_dev) == 1
    assert torch.equal(oa.flat, ob.flat)
    ob.skip_nonfinite = False  # settable afterwards: back to today's single call
    ob.max_grad_norm = None
    for o, ps in ((oa, a), (ob, b)):
        _set(ps, _grads(2))
        o.step()
    assert torch.equal(oa.flat, ob.flat)


# 7 -- accumulation at the optimizer ------------------------------------------------------------
def test_accumulated_micro_gradients():
    """Three micro-gradient sets per update, two updates.  Tensor 1 misses micro-step 1 (it is
    stepped, the missing one counts as zeros); tensor 3 misses all three (not stepped, no
    state); tensor 0 misses the FIRST micro-step (the gather writes its zeros)."""
    from e2ep_amd.optim import FlatAdam
    ps = _params(7)
    opt = FlatAdam(ps, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    flat = torch.full((opt.numel,), 7.0, device=DEV)  # stale contents: the gather overwrites
    has = torch.zeros(len(ps), dtype=torch.int64, device=DEV)
    before3 = ps[3].detach().clone()
    means = []
    for cycle in range(2):
        micro = []
        for j in range(3):
            gs = _grads(10 * cycle + j)
            gs[3] = None
            if j == 1:
                gs[1] = None
            if j == 0:
                gs[0] = None
            micro.append(gs)
            _set(ps, gs)
            opt.prepare()
            opt.accumulate_grads(flat, first=j == 0)
            opt.has_grad(has, union=j > 0)
        assert has.cpu().tolist() == [1, 1, 1, 0, 1, 1, 1]
        mean = []
        for i, (o, n) in enumerate(opt.spans):
            parts = [m[i] for m in micro if m[i] is not None]
            if not parts:
                assert not flat[o:o + n].any()
                mean.append(None)
                continue
            want = torch.zeros_like(parts[0]) if micro[0][i] is None else None
            for x in parts:  # the same order, with torch on the device
                want = x.clone() if want is None else want + x
            assert torch.equal(flat[o:o + n], want.reshape(-1)), i
            mean.append(sum(x.cpu().double() for x in parts) / 3.0)
        means.append(mean)
        opt.step(flat, 1.0 / 3.0, has_grad=has)
    ref, topt, norms = _ref_chain(7, means, 1.0, 1e-4)
    # fp32 sums of three values and the fp32 1/3 (3e-8 off) against the exact mean: under an ulp
    assert abs(float(opt.grad_norm_dev) - norms[-1]) / norms[-1] <= ULP
    for i, (p, q) in enumerate(zip(ref, ps)):
        assert rel_l2(q.detach(), p.detach()) < 1e-6, i
    assert torch.equal(ps[3].detach(), before3)
    assert sorted(opt.state_dict()["state"]) == sorted(topt.state_dict()["state"]) == [0, 1, 2, 4, 5, 6]


# 8 -- TrainStep on the MLP ---------------------------------------------------------------------
class _Small(torch.nn.Module):
    """cut=True declares one cut point between the layers (the identity outside
    segments.record()), so a graph-mode data-parallel TrainStep takes the segmented backward."""

    def __init__(self, cut=False):
        super().__init__()
        torch.manual_seed(3)
        self.a = torch.nn.Linear(16, 32)
        self.b = torch.nn.Linear(32, 4)
        self.cut = cut

    def training_step(self, batch, idx=0):
        from e2ep_amd import segments
        h = self.a(batch["x"]).relu()
        if self.cut:
            h = segments.cut(h)
        return (self.b(h) - batch["y"]).pow(2).mean()


def _small_batch(seed):
    g = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(8, 16, generator=g).to(DEV), "y": torch.randn(8, 4, generator=g).to(DEV)}


def _flat(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()


_CLIP = 0.05  # the MLP's gradient norm is about 1: every update is clipped


def _mlp_run(graph, **kw):
    """Two warm-up micro-steps on the construction batch (one cycle; the graph-mode constructor
    makes them itself), then four calls on alternating batches.  Returns losses, the parameters
    after every call, the step object and the module."""
    from e2ep_amd.train import TrainStep
    m = _Small().to(DEV)
    s = TrainStep(m, _small_batch(1), graph=graph, warmup=2, max_grad_norm=_CLIP, accumulate=2,
                  **kw)
    if not graph:
        s(), s()
    losses, after = [], [_flat(m)]
    for k in range(4):
        losses.append(float(s(_small_batch(2 + k % 2))))
        after.append(_flat(m))
    return losses, after, s, m


def test_train_step_mlp_clip_and_accumulate():
    le, ae, se, _ = _mlp_run(False)
    lg, ag, sg, _ = _mlp_run(True)
    assert sg.g_acc is not None and sg.g_gather is not None and sg.g_opt is not None
    assert le == lg
    for k in range(4):  # parameters change on calls 2 and 4 only
        for after in (ae, ag):
            assert torch.equal(after[k], after[k + 1]) == (k % 2 == 0)
    assert float(sg.grad_norm) > _CLIP and float(sg.opt.clip_coef_dev) < 1.0
    assert sg.grad_norm.data_ptr() == sg.opt.grad_norm_dev.data_ptr()
    assert float(sg.grad_norm) == float(se.grad_norm)
    # graph vs eager: the bound is 1e-6; the same kernels run on the same values, and the
    # runs were observed bitwise equal
    assert rel_l2(ag[-1], ae[-1]) < 1e-6
    assert torch.equal(ag[-1], ae[-1])
    # plain torch on the device: two backward passes, mean, clip_grad_norm_, Adam
    m = _Small().to(DEV)
    topt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=1e-4, foreach=False)
    batches = [_small_batch(1)] * 2 + [_small_batch(2 + k % 2) for k in range(4)]
    for c in range(3):
        topt.zero_grad(set_to_none=True)
        for b in batches[2 * c:2 * c + 2]:
            m.training_step(b).backward()
        for p in m.parameters():
            p.grad.div_(2.0)
        torch.nn.utils.clip_grad_norm_(m.parameters(), _CLIP, foreach=False)
        topt.step()
    assert rel_l2(ag[-1], _flat(m)) < 1e-6 and rel_l2(ae[-1], _flat(m)) < 1e-6


def test_train_step_default_options_change_nothing():
    from e2ep_amd.train import TrainStep
    out = []
    for kw in ({}, dict(max_grad_norm=None, skip_nonfinite=False, accumulate=1)):
        m = _Small().to(DEV)
        s = TrainStep(m, _small_batch(1), graph=True, warmup=1, **kw)
        assert s.flat_grad is None and s.g_gather is None and s.g_acc is None
        for _ in range(3):
            s()
        out.append(_flat(m))
    assert torch.equal(out[0], out[1])
    # a passed-in optimizer keeps its own settings unless an argument is given: an explicit
    # skip_nonfinite=False switches the skip off, max_grad_norm=None means "not given"
    from e2ep_amd.optim import FlatAdam
    m = _Small().to(DEV)
    opt = FlatAdam(list(m.parameters()), lr=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    TrainStep(m, _small_batch(1), graph=False, optimizer=opt)
    assert opt.max_grad_norm == 1.0 and opt.skip_nonfinite is True
    TrainStep(m, _small_batch(1), graph=False, optimizer=opt, skip_nonfinite=False,
              max_grad_norm=None)
    assert opt.max_grad_norm == 1.0 and opt.skip_nonfinite is False
    TrainStep(m, _small_batch(1), graph=False, optimizer=opt, max_grad_norm=0.5)
    assert opt.max_grad_norm == 0.5


# 9 -- TrainStep on the full model --------------------------------------------------------------
def test_train_step_full_model_graph_matches_eager():
    from e2ep_amd import synthetic
    from e2ep_amd.train import TrainStep
    from test_train_step_gpu import _batch, _module
    noise = synthetic.target_noise(2, seed=7).to(DEV)
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True, accumulate=2)
    m_e, m_g = _module(noise), _module(noise)
    s_e = TrainStep(m_e, _batch(2), graph=False, **kw)
    s_g = TrainStep(m_g, _batch(2), graph=True, warmup=2, **kw)
    for _ in range(2):
        s_e()
    losses_e = [float(s_e()) for _ in range(4)]
    losses_g = [float(s_g()) for _ in range(4)]
    for a, b in zip(losses_e, losses_g):
        assert abs(a / b - 1) < 1e-6, (losses_e, losses_g)
    assert losses_g[2] != losses_g[0]  # the replayed update really moves the weights
    pe = dict(m_e.named_parameters())
    for k, p in m_g.named_parameters():
        assert rel_l2(p.detach(), pe[k].detach()) < 1e-6, k
    assert int(s_g.opt.skipped_dev) == 0 and int(s_e.opt.skipped_dev) == 0
    print(f"norm {float(s_g.grad_norm)!r} coefficient {float(s_g.opt.clip_coef_dev)!r}")
    assert float(s_g.opt.clip_coef_dev) < 1.0  # this model's gradient norm is about 40
    assert abs(float(s_g.grad_norm) / float(s_e.grad_norm) - 1) < 1e-6


# 10 -- data-parallel form ----------------------------------------------------------------------
def _port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def test_rccl_world1_clip_and_accumulate_are_exact():
    from e2ep_amd.train import TrainStep
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV, 0))
    try:
        for graph in (True, False):
            _, a_ref, _, _ = _mlp_run(graph)
            _, a_ddp, s, _ = _mlp_run(graph, ddp=True)
            assert s.segmented is False and s.buckets is None and s.ddp
            assert torch.equal(a_ref[-1], a_ddp[-1]) and not torch.equal(a_ddp[0], a_ddp[-1])
        # accumulate = 1: the segmented graph path (the MLP with a cut point between its layers:
        # stage graphs, the buckets all-reduced between their replays, the optimizer graph)
        # still clips, and equals the run without ddp
        out = []
        for cut, kw in ((False, {}), (True, {}), (True, dict(ddp=True))):
            m = _Small(cut=cut).to(DEV)
            s = TrainStep(m, _small_batch(1), graph=True, warmup=1, max_grad_norm=_CLIP, **kw)
            if kw:
                assert s.segmented and s.g_bwd is None and s.g_s2 is not None
                assert s.g_s1g is not None and s.g_s2g is not None and s.g_opt is not None
            else:
                assert not s.segmented and s.g_bwd is not None
            for k in range(3):
                s(_small_batch(2 + k % 2))
            assert float(s.grad_norm) > _CLIP and float(s.opt.clip_coef_dev) < 1.0
            out.append(_flat(m))
        assert torch.equal(out[0], out[1]) and torch.equal(out[1], out[2])
    finally:
        torch.cuda.synchronize()  # no queued work on any stream when the communicator goes
        dist.destroy_process_group()
