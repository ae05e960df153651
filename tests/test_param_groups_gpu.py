"""FlatAdam with parameter groups (csrc/adam.hip: k_adam_groups; e2ep_amd/optim.py) on the device.

Three groups interleaved in layout order, A = {0, 2, 5}, B = {1, 4}, C = {3, 6}, over
test_optim_gpu.py's SHAPES: neighbouring tensors differ in group, and the 4097- and 20000-element
tensors span 2 and 5 chunk-table rows, each of which has to carry its tensor's group.

Against torch.optim.Adam the bound is rel_l2 < 1e-6 per tensor, the bound
test_flat_adam_matches_torch_adam holds the same fp32 chain to (a CPU fp32 restatement of the
grouped arithmetic agrees with torch to 2.2e-9 on these inputs).  Everything else is compared
bit for bit."""
import importlib
import os
import types

import pytest
import torch

from helpers import rel_l2
from test_optim_gpu import SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
GROUPS = {"A": (0, 2, 5), "B": (1, 4), "C": (3, 6)}
# distinct learning rates, L2 and decoupled weight decay mixed
HYPER = {"A": dict(lr=1e-3, weight_decay=1e-4, decoupled_weight_decay=False),
         "B": dict(lr=3e-4, weight_decay=1e-2, decoupled_weight_decay=True),
         "C": dict(lr=2e-3, weight_decay=0.0, decoupled_weight_decay=False)}
SAME = dict(lr=1e-3, weight_decay=1e-4, decoupled_weight_decay=False)
MODES = {"plain": {}, "clip": dict(max_grad_norm=1.0, skip_nonfinite=True),
         "ema": dict(ema_decay=0.9, ema_warmup=True),
         "both": dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9, ema_warmup=True)}


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(DEV).requires_grad_() for s in SHAPES]


def _grads(step, skip=()):
    g = torch.Generator().manual_seed(100 + step)
    return [None if i in skip else torch.randn(s, generator=g).to(DEV) for i, s in enumerate(SHAPES)]


def _set(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.clone()


def _groups(ps, hyper=HYPER):
    """A, B and C over `ps`; `hyper` is per group (HYPER) or one dict for all three (SAME)."""
    return [dict(params=[ps[i] for i in idx], name=n, **(hyper[n] if n in hyper else hyper))
            for n, idx in GROUPS.items()]


def _record(monkeypatch):
    from e2ep_amd import _lib
    names, orig = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return orig(name, *args)

    monkeypatch.setattr(_lib, "call", recording)
    return names


def _flat_step(opt, flat, has, scale=2.0):
    """The data-parallel form: gathered, summed over `scale` identical ranks, stepped with
    1 / scale and the has_grad vector."""
    opt.prepare()
    opt.gather_grads(flat)
    flat.mul_(scale)
    opt.has_grad(has)
    opt.step(flat, 1.0 / scale, has_grad=has)


# 1 -- against torch ----------------------------------------------------------------------------
def test_grouped_flat_adam_matches_torch_adam_under_a_schedule():
    from e2ep_amd.optim import FlatAdam
    ref, mine = _params(0), _params(0)
    topt = torch.optim.Adam(_groups(ref), foreach=False)
    fopt = FlatAdam(_groups(mine), order=mine)
    assert fopt.grouped and fopt.n_groups == 3 and fopt.params == mine
    rows = fopt.chunks.view(-1, 4).cpu().tolist()
    assert [r[3] for r in rows] == [fopt.group_of[r[0]] for r in rows]
    assert fopt.group_of == [0, 1, 0, 2, 1, 0, 2]
    assert sum(1 for r in rows if r[0] == 2) == 2 and sum(1 for r in rows if r[0] == 5) == 5
    assert fopt.wd_dev.cpu().tolist() == [1e-4, 1e-2, 0.0]
    assert fopt.flags_dev.cpu().tolist() == [0, 1, 0]
    ts = torch.optim.lr_scheduler.CosineAnnealingLR(topt, T_max=4)
    fs = torch.optim.lr_scheduler.CosineAnnealingLR(fopt, T_max=4)
    seen = []
    for k in range(6):
        gs = _grads(k)
        _set(ref, gs)
        _set(mine, gs)
        topt.step()
        fopt.step()
        lrs = [g["lr"] for g in fopt.param_groups]
        assert lrs == [g["lr"] for g in topt.param_groups]
        assert fopt.lr_dev.cpu().tolist() == lrs  # every group's own schedule reached the device
        seen.append(tuple(lrs))
        ts.step()
        fs.step()
        for i, (p, q) in enumerate(zip(ref, mine)):
            err = rel_l2(q.detach(), p.detach())
            print("groups_vs_torch", k, i, f"{err:.3e}")
            assert err < 1e-6, (k, i, err)
    assert seen[0] == (1e-3, 3e-4, 2e-3) and all(len(set(lrs)) == 3 for lrs in seen[:4])
    assert all(x > y for a, b in zip(seen[:4], seen[1:5]) for x, y in zip(a, b))  # annealing
    sd, tsd = fopt.state_dict(), topt.state_dict()
    cat = [i for idx in GROUPS.values() for i in idx]  # torch's numbering: the groups concatenated
    for t, i in enumerate(cat):
        assert float(sd["state"][t]["step"]) == float(tsd["state"][t]["step"]) == 6.0
        assert sd["state"][t]["exp_avg_sq"].shape == SHAPES[i]
        assert rel_l2(sd["state"][t]["exp_avg_sq"], tsd["state"][t]["exp_avg_sq"]) < 1e-6
        assert rel_l2(sd["state"][t]["exp_avg"], tsd["state"][t]["exp_avg"]) < 1e-6


# 2 -- grouped equals ungrouped, bitwise --------------------------------------------------------
@pytest.mark.parametrize("path", ["table", "flat"])
@pytest.mark.parametrize("mode", list(MODES))
def test_grouped_equals_ungrouped_bitwise(mode, path, monkeypatch):
    from e2ep_amd.optim import FlatAdam
    kw = MODES[mode]
    a, b = _params(1), _params(1)
    plain = FlatAdam(a, **{k: v for k, v in SAME.items() if k != "decoupled_weight_decay"}, **kw)
    grouped = FlatAdam(_groups(b, SAME), order=b, **kw)
    assert grouped.grouped and not plain.grouped
    names = _record(monkeypatch)
    flats = [torch.zeros(plain.numel, device=DEV) for _ in range(2)]
    has = [torch.zeros(len(a), dtype=torch.int64, device=DEV) for _ in range(2)]
    for k in range(3):
        gs = _grads(k, skip=(4,) if k == 1 else ())
        for n, (ps, opt) in enumerate(((a, plain), (b, grouped))):
            _set(ps, gs)
            if path == "table":
                opt.step()
            else:
                _flat_step(opt, flats[n], has[n])
    assert "e2ep_adam_step_groups" in names
    assert torch.equal(grouped.flat, plain.flat)
    assert torch.equal(grouped.exp_avg, plain.exp_avg)
    assert torch.equal(grouped.exp_avg_sq, plain.exp_avg_sq)
    assert torch.equal(grouped.step_count, plain.step_count)
    assert torch.equal(grouped.stepped, plain.stepped)
    if "ema_decay" in kw:
        assert torch.equal(grouped.ema, plain.ema) and not torch.equal(plain.ema, plain.flat)
        assert torch.equal(grouped.ema_updates_dev, plain.ema_updates_dev)
    if "max_grad_norm" in kw:
        assert torch.equal(grouped.grad_norm_dev, plain.grad_norm_dev)
        assert torch.equal(grouped.clip_coef_dev, plain.clip_coef_dev)
        assert float(plain.clip_coef_dev) < 1.0  # the clipping really acted


# 3 -- grouped equals one optimizer per group, bitwise ------------------------------------------
@pytest.mark.parametrize("ema", [False, True])
def test_grouped_equals_independent_optimizers_bitwise(ema):
    from e2ep_amd.optim import FlatAdam
    kw = dict(ema_decay=0.9, ema_warmup=True) if ema else {}
    a, b = _params(2), _params(2)
    grouped = FlatAdam(_groups(a), order=a, **kw)
    alone = {n: FlatAdam([b[i] for i in idx], **HYPER[n], **kw) for n, idx in GROUPS.items()}
    assert [o.grouped for o in alone.values()] == [False, True, False]
    for k in range(3):
        gs = _grads(k)
        _set(a, gs)
        _set(b, gs)
        grouped.step()
        for o in alone.values():
            o.step()
    for n, idx in GROUPS.items():
        o = alone[n]
        for j, i in enumerate(idx):
            (go, gn), (oo, on) = grouped.spans[i], o.spans[j]
            assert torch.equal(a[i].detach(), b[i].detach()), (n, i)
            assert torch.equal(grouped.exp_avg[go:go + gn], o.exp_avg[oo:oo + on]), (n, i)
            assert torch.equal(grouped.exp_avg_sq[go:go + gn], o.exp_avg_sq[oo:oo + on]), (n, i)
            if ema:
                assert torch.equal(grouped.ema_param(i), o.ema_param(j)), (n, i)
                assert not torch.equal(grouped.ema_param(i), a[i].detach())


# 4 -- gradient sources -------------------------------------------------------------------------
def test_grouped_unaligned_gradient_equals_aligned_bitwise():
    from e2ep_amd.optim import FlatAdam
    kw = dict(ema_decay=0.9)
    a, b = _params(3), _params(3)
    oa, ob = FlatAdam(_groups(a), order=a, **kw), FlatAdam(_groups(b), order=b, **kw)
    for k in range(3):
        gs = _grads(k)
        _set(a, gs)
        _set(b, gs)
        for i in (2, 4):  # an L2 tensor of two rows and a decoupled one
            buf = torch.zeros(gs[i].numel() + 8, device=DEV)
            b[i].grad = buf[1:1 + gs[i].numel()].copy_(gs[i].view(-1)).view(SHAPES[i])
            assert b[i].grad.data_ptr() % 16 == 4 and a[i].grad.data_ptr() % 16 == 0
        oa.step()
        ob.step()
    for t in ("flat", "exp_avg", "exp_avg_sq", "ema"):
        assert torch.equal(getattr(oa, t), getattr(ob, t)), t


@pytest.mark.parametrize("mode", ["ema", "both"])
def test_grouped_gathered_gradients_equal_table_gradients_bitwise(mode):
    """Step 1 leaves tensor 4 (group B, decoupled) without a gradient on both paths: not
    stepped, not decayed, and its average still moves."""
    from e2ep_amd.optim import FlatAdam
    kw = MODES[mode]
    a, b = _params(4), _params(4)
    oa, ob = FlatAdam(_groups(a), order=a, **kw), FlatAdam(_groups(b), order=b, **kw)
    flat = torch.zeros(ob.numel, device=DEV)
    has = torch.zeros(len(b), dtype=torch.int64, device=DEV)
    o4, n4 = oa.spans[4]
    for k in range(3):
        gs = _grads(k, skip=(4,) if k == 1 else ())
        _set(a, gs)
        _set(b, gs)
        before = [t[o4:o4 + n4].clone() for t in (oa.flat, oa.exp_avg, oa.exp_avg_sq, oa.ema)]
        oa.step()
        _flat_step(ob, flat, has)
        after = [t[o4:o4 + n4] for t in (oa.flat, oa.exp_avg, oa.exp_avg_sq, oa.ema)]
        if k == 1:
            assert all(torch.equal(x, y) for x, y in zip(before[:3], after[:3]))
            assert not torch.equal(before[3], after[3])  # the average moved toward the kept p
            want = torch.addcmul(before[3].double(), before[0].double() - before[3].double(),
                                 torch.tensor(1.0 - min(0.9, 3 / 12), dtype=torch.float64, device=DEV))
            assert rel_l2(after[3], want) < 1e-6
        else:
            assert not any(torch.equal(x, y) for x, y in zip(before, after))
    for t in ("flat", "exp_avg", "exp_avg_sq", "ema", "stepped", "step_count"):
        assert torch.equal(getattr(oa, t), getattr(ob, t)), t
    if mode == "both":
        assert torch.equal(oa.grad_norm_dev, ob.grad_norm_dev)


@pytest.mark.parametrize("clip", [None, 1.0])
def test_grouped_nonfinite_step_changes_nothing_in_any_group(clip):
    from e2ep_amd.optim import FlatAdam
    ps = _params(5)
    opt = FlatAdam(_groups(ps), order=ps, max_grad_norm=clip, skip_nonfinite=True, ema_decay=0.9,
                   ema_warmup=True)

    def state():
        return [t.clone() for t in (opt.ema, opt.ema_updates_dev, opt.flat, opt.exp_avg,
                                    opt.exp_avg_sq, opt.step_count, opt.stepped)]

    _set(ps, _grads(0))
    opt.step()
    s0 = state()
    gs = _grads(1)
    gs[1].view(-1)[7] = float("inf")  # one element of one group-B tensor
    _set(ps, gs)
    opt.step()
    for t0, t1 in zip(s0, state()):
        assert torch.equal(t0, t1)
    assert int(opt.skipped_dev) == 1
    _set(ps, _grads(2))
    opt.step()
    assert all(not torch.equal(t0, t1) for t0, t1 in zip(s0[:6], state()[:6]))
    assert int(opt.skipped_dev) == 1 and float(opt.step_count) == 2.0


# 5 -- entry point ------------------------------------------------------------------------------
def test_entry_point_calls_with_and_without_groups(monkeypatch):
    from e2ep_amd.optim import FlatAdam
    cases = [(lambda ps: FlatAdam(_groups(ps), order=ps), ["e2ep_adam_step_groups"]),
             (lambda ps: FlatAdam([dict(params=ps, lr=1e-3)]), ["e2ep_adam_step"]),
             (lambda ps: FlatAdam(ps, lr=1e-3, weight_decay=1e-2), ["e2ep_adam_step"]),
             (lambda ps: FlatAdam(ps, lr=1e-3, weight_decay=1e-2, decoupled_weight_decay=True),
              ["e2ep_adam_step_groups"]),
             (lambda ps: FlatAdam(_groups(ps), order=ps, max_grad_norm=1.0, ema_decay=0.9),
              ["e2ep_grad_sqnorm", "e2ep_grad_norm_finalize", "e2ep_adam_step_groups"])]
    opts = [(build(_params(6)), want) for build, want in cases]
    names = _record(monkeypatch)
    for opt, want in opts:
        _set(opt.params, _grads(0))
        del names[:]
        opt.step()
        assert names == want
    # one decoupled group is AdamW
    ref = _params(6)
    topt = torch.optim.AdamW(ref, lr=1e-3, weight_decay=1e-2, foreach=False)
    _set(ref, _grads(0))
    topt.step()
    for p, q in zip(ref, opts[3][0].params):
        assert rel_l2(q.detach(), p.detach()) < 1e-6
    assert not torch.equal(opts[3][0].flat, opts[2][0].flat)


def test_entry_point_refuses_bad_group_tables():
    from e2ep_amd import _lib
    from e2ep_amd.optim import FlatAdam
    ps = _params(6)
    opt = FlatAdam(_groups(ps), order=ps)
    _set(ps, _grads(0))
    opt.prepare()
    before = opt.flat.clone()
    einval = _lib.CONSTANTS["E2EP_EINVAL"]

    def call(lr=opt.lr_dev, wd=opt.wd_dev, flags=opt.flags_dev, n=opt.n_groups):
        return _lib.call_raw(
            "e2ep_adam_step_groups", _lib.ptr(opt.chunks), opt.n_chunks, _lib.ptr(opt.offsets),
            _lib.ptr(opt._gtab), None, _lib.ptr(opt.flat), _lib.ptr(opt.exp_avg),
            _lib.ptr(opt.exp_avg_sq), _lib.ptr(opt.step_count), _lib.ptr(lr), _lib.ptr(wd),
            _lib.ptr(flags), n, 0.9, 0.999, 1e-8, 1.0, None, None, _lib.ptr(opt.stepped), None,
            None, 0.0, 0, _lib.stream())

    for kw in (dict(n=0), dict(n=-1), dict(lr=None), dict(wd=None), dict(flags=None)):
        assert call(**kw) == einval, kw
    assert torch.equal(opt.flat, before) and float(opt.step_count) == 0.0
    assert call() == 0
    assert not torch.equal(opt.flat, before) and float(opt.step_count) == 1.0


# 6 -- guard bands ------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["table", "flat"])
def test_guarded_grouped_step(path):
    """test_guarded_ema_step_and_swap's way: two clipped, averaged, grouped steps (step 1 leaves
    tensor 4 without a gradient) with every flat buffer, the group tables and the device scalars
    in arenas, unguarded and under both fills; then a step of an optimizer whose rows of the
    4097-element tensor carry group id n_groups: that tensor is left as it is."""
    G = importlib.import_module("test_guarded_ops_gpu")
    from e2ep_amd.optim import FlatAdam
    g = G._g(43)
    p0 = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(2)]
    grads[1][4] = None
    ref = [p.double().requires_grad_() for p in p0]
    topt = torch.optim.Adam(_groups(ref), foreach=False)
    for step in grads:
        for p, a in zip(ref, step):
            p.grad = None if a is None else a.double()
        torch.nn.utils.clip_grad_norm_(ref, 0.5, foreach=False)
        topt.step()

    def fn():
        ps = [G._put(p, True) for p in p0]
        opt = FlatAdam(_groups(ps), order=ps, max_grad_norm=0.5, ema_decay=0.9, ema_warmup=True)
        flat = torch.empty(opt.numel, device=DEV) if path == "flat" else None
        has = torch.zeros(len(ps), dtype=torch.int64, device=DEV)

        def step(o, gs):
            for p, a in zip(o.params, gs):
                p.grad = None if a is None else G._put(a)
            if path == "table":
                o.step()
            else:
                o.prepare()
                o.gather_grads(flat)
                o.has_grad(has)
                o.step(flat, 1.0, has_grad=has)

        for gs in grads:
            step(opt, gs)
        for q, r in zip(ps, ref):
            assert rel_l2(q.detach(), r.detach()) < 1e-6
        # a row whose group is n_groups: never indexes the tables, leaves its tensor alone
        qs = [G._put(p, True) for p in p0]
        bad = FlatAdam(_groups(qs), order=qs, max_grad_norm=0.5, ema_decay=0.9, ema_warmup=True)
        r0, r1 = bad.chunk_rows[2]
        assert r1 - r0 == 2
        bad.chunks.view(-1, 4)[r0:r1, 3] = bad.n_groups
        step(bad, grads[0])
        o2, n2 = bad.spans[2]
        assert torch.equal(qs[2].detach().cpu(), p0[2])
        assert torch.equal(bad.ema[o2:o2 + n2].cpu(), p0[2])
        assert not bool(bad.exp_avg[o2:o2 + n2].any()) and not bool(bad.exp_avg_sq[o2:o2 + n2].any())
        assert int(bad.stepped[2]) == 0 and int(bad.stepped.sum()) == len(qs) - 1
        assert all(not torch.equal(q.detach().cpu(), p) for i, (q, p) in enumerate(zip(qs, p0))
                   if i != 2)
        return dict(flat=opt.flat, ema=opt.ema, exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq,
                    steps=opt.step_count, updates=opt.ema_updates_dev, coef=opt.clip_coef_dev,
                    partials=opt._partials, lr=opt.lr_dev, wd=opt.wd_dev, flags=opt.flags_dev,
                    bad_flat=bad.flat, bad_ema=bad.ema, bad_exp_avg=bad.exp_avg,
                    bad_exp_avg_sq=bad.exp_avg_sq)

    G.run_guarded(fn, "flat_adam_groups")


# 7 -- state ------------------------------------------------------------------------------------
ORDER = (4, 0, 6, 2, 5, 1, 3)   # the flat layout: no group is contiguous in it
ORDER2 = (3, 6, 1, 0, 5, 4, 2)


def _clones(ps):
    return [p.detach().clone().requires_grad_() for p in ps]


def test_state_round_trips_through_torch_and_through_itself():
    from e2ep_amd.optim import FlatAdam
    ref, mine = _params(7), _params(7)
    topt = torch.optim.Adam(_groups(ref), foreach=False)
    fopt = FlatAdam(_groups(mine), order=[mine[i] for i in ORDER])
    assert [id(p) for p in fopt.params] == [id(mine[i]) for i in ORDER]
    for k in range(2):
        _set(ref, _grads(k))
        _set(mine, _grads(k))
        topt.step()
        fopt.step()
    sd, tsd = fopt.state_dict(), topt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2], [3, 4], [5, 6]]
    assert [g["params"] for g in tsd["param_groups"]] == [[0, 1, 2], [3, 4], [5, 6]]
    for g, n in zip(sd["param_groups"], GROUPS):
        assert g["name"] == n
        for key, v in HYPER[n].items():
            assert g[key] == v, (n, key)
    cat = [i for idx in GROUPS.values() for i in idx]
    assert sorted(sd["state"]) == list(range(7))
    for t, i in enumerate(cat):
        assert sd["state"][t]["exp_avg"].shape == SHAPES[i]
    # FlatAdam -> torch.optim.Adam, torch.optim.Adam -> FlatAdam, FlatAdam -> FlatAdam (in
    # another layout), each from the weights after step 2
    t2p, f2p, f3p = _clones(mine), _clones(ref), _clones(mine)
    t2 = torch.optim.Adam(_groups(t2p), foreach=False)
    t2.load_state_dict(sd)
    f2 = FlatAdam(_groups(f2p, SAME), order=[f2p[i] for i in ORDER])  # other hyper-parameters
    f2.load_state_dict(tsd)
    f3 = FlatAdam(_groups(f3p, SAME), order=[f3p[i] for i in ORDER2])
    f3.load_state_dict(sd)
    for o in (f2, f3):
        assert o.wd_dev.cpu().tolist() == [1e-4, 1e-2, 0.0] and o.flags_dev.cpu().tolist() == [0, 1, 0]
        assert [g["lr"] for g in o.param_groups] == [1e-3, 3e-4, 2e-3]
        assert float(o.step_count) == 2.0 and int(o.stepped.sum()) == 7
    for ps in (ref, mine, t2p, f2p, f3p):
        _set(ps, _grads(2))
    for o in (topt, fopt, t2, f2, f3):
        o.step()
    assert f2.lr_dev.cpu().tolist() == [1e-3, 3e-4, 2e-3]
    for i in range(7):
        for name, ps in (("flat->torch", t2p), ("torch->flat", f2p), ("flat->flat", f3p), ("flat", mine)):
            err = rel_l2(ps[i].detach(), ref[i].detach())
            print("round_trip", name, i, f"{err:.3e}")
            assert err < 1e-6, (name, i, err)
        assert torch.equal(f3p[i].detach(), mine[i].detach())  # the layout changes no bit
    assert rel_l2(f3.state_dict()["state"][3]["exp_avg_sq"], topt.state_dict()["state"][3]["exp_avg_sq"]) < 1e-6
    # a tensor that was never stepped has no state, under its torch index
    ps = _params(7)
    o = FlatAdam(_groups(ps), order=[ps[i] for i in ORDER])
    _set(ps, _grads(0, skip=(4,)))
    o.step()
    assert sorted(o.state_dict()["state"]) == [t for t, i in enumerate(cat) if i != 4]
    with pytest.raises(ValueError, match="parameter groups"):
        FlatAdam(_params(7)).load_state_dict(sd)


def test_one_group_state_is_what_it_was():
    from e2ep_amd.optim import FlatAdam
    ps = _params(7)
    o = FlatAdam(ps, lr=1e-3, weight_decay=1e-4)
    _set(ps, _grads(0))
    o.step()
    sd = o.state_dict()
    assert list(sd["param_groups"][0]) == ["lr", "betas", "eps", "weight_decay", "amsgrad", "maximize",
                                           "foreach", "capturable", "differentiable", "fused", "params"]
    assert sd["param_groups"][0]["params"] == list(range(7)) and list(sd["state"]) == list(range(7))


def test_constructor_errors():
    from e2ep_amd.optim import FlatAdam
    ps = _params(8)
    with pytest.raises(ValueError, match="more than one"):
        FlatAdam([dict(params=ps[:4]), dict(params=ps[3:])])
    with pytest.raises(ValueError, match="order"):
        FlatAdam(_groups(ps), order=ps[:-1])
    with pytest.raises(ValueError, match="order"):
        FlatAdam(_groups(ps), order=ps[:-1] + _params(8)[-1:])
    with pytest.raises(ValueError, match="order"):
        FlatAdam(_groups(ps), order=ps + ps[:1])
    with pytest.raises(ValueError, match="betas"):
        FlatAdam([dict(params=ps[:4]), dict(params=ps[4:], betas=(0.8, 0.999))])
    with pytest.raises(ValueError, match="eps"):
        FlatAdam([dict(params=ps[:4], eps=1e-6), dict(params=ps[4:])])
    opt = FlatAdam([dict(params=ps[:4]), dict(params=ps[4:], lr=1e-2)])
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 1e-2] and opt.lr == 1e-3
    assert opt.params == ps  # default layout: the groups concatenated
    with pytest.raises(ValueError, match="layout"):
        opt.add_param_group(dict(params=_params(8)[:1]))
    opt.lr = 5e-4
    assert opt.param_groups[0]["lr"] == 5e-4 and opt.param_groups[1]["lr"] == 1e-2


# 8 -- TrainStep on an MLP ----------------------------------------------------------------------
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


def _small_opt(m, order=None):
    from e2ep_amd.optim import FlatAdam
    groups = [dict(params=list(m.a.parameters()), lr=1e-2, name="a"),
              dict(params=list(m.b.parameters()), lr=3e-3, weight_decay=1e-2,
                   decoupled_weight_decay=True, name="b")]
    return FlatAdam(groups, weight_decay=1e-4,
                    order=list(m.parameters()) if order is None else order)


def _mlp_run(graph, calls, **kw):
    """Two warm-up calls on the construction batch (the graph-mode constructor makes them
    itself), then `calls` calls on alternating batches, a scheduler step and sync_lr between
    calls."""
    from e2ep_amd.train import TrainStep
    m = _Small().to(DEV)
    opt = _small_opt(m)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=4)
    s = TrainStep(m, _small_batch(1), graph=graph, warmup=2, optimizer=opt, **kw)
    if not graph:
        s(), s()
    for k in range(calls):
        sched.step()
        opt.sync_lr()
        s(_small_batch(2 + k % 2))
    return s


@pytest.mark.parametrize("accumulate", [1, 2])
def test_train_step_captured_equals_eager_with_groups(accumulate):
    calls = 5 if accumulate == 1 else 6
    se, sg = _mlp_run(False, calls, accumulate=accumulate), _mlp_run(True, calls, accumulate=accumulate)
    assert sg.g_opt is not None and sg.opt.grouped and sg.opt.n_groups == 2
    for t in ("flat", "exp_avg", "exp_avg_sq", "step_count", "lr_dev"):
        assert torch.equal(getattr(sg.opt, t), getattr(se.opt, t)), t
    assert float(sg.opt.step_count) == (2 + calls) // accumulate
    lrs = sg.opt.lr_dev.cpu().tolist()
    assert lrs == [g["lr"] for g in sg.opt.param_groups] and lrs[0] != 1e-2 and lrs[1] != 3e-3
    fresh = _Small().to(DEV)
    assert not any(torch.equal(p.detach(), q.detach()) for p, q in zip(sg.module.parameters(), fresh.parameters()))


def test_train_step_checks_a_grouped_optimizers_layout():
    from e2ep_amd.train import TrainStep
    m = _Small().to(DEV)
    opt = _small_opt(m, order=list(m.parameters())[::-1])
    with pytest.raises(ValueError, match="order"):
        TrainStep(m, _small_batch(1), graph=False, optimizer=opt)
    # the optimizer TrainStep builds itself follows module.cfg's keys
    m = _Small().to(DEV)
    m.cfg = types.SimpleNamespace(no_decay_norm_bias=True, decoupled_weight_decay=True)
    o = TrainStep(m, _small_batch(1), graph=False, lr=1e-3, weight_decay=1e-2).opt
    assert [g["name"] for g in o.param_groups] == ["rest_decay", "rest_no_decay"]
    assert o.wd_dev.cpu().tolist() == [1e-2, 0.0] and o.flags_dev.cpu().tolist() == [1, 1]
    assert o.group_of == [0, 1, 0, 1] and all(a is b for a, b in zip(o.params, m.parameters()))
    o = TrainStep(_Small().to(DEV), _small_batch(1), graph=False).opt
    assert not o.grouped and len(o.param_groups) == 1


# 9 -- full model -------------------------------------------------------------------------------
def _full_module():
    from tool.config import default_cfg
    from trainer.pl_trainer import ParkingTrainingModule
    from weights import make_state
    mod = ParkingTrainingModule(default_cfg(deterministic=True, backbone_lr_scale=0.1,
                                            no_decay_norm_bias=True, decoupled_weight_decay=True))
    mod.parking_model.load_state_dict(make_state(mod.parking_model.state_dict(), 1234))
    mod = mod.to(DEV)
    for p in mod.parking_model.bev_encoder.layer4.parameters():
        p.requires_grad_(False)
    return mod.train()


def test_full_model_recipe_steps_and_round_trips_a_checkpoint(tmp_path):
    from e2ep_amd import checkpoint, synthetic
    from e2ep_amd.optim import FlatAdam
    from e2ep_amd.train import TrainStep
    m = _full_module()
    out = m.configure_optimizers()
    opt, sched = out["optimizer"], out["lr_scheduler"]
    lr, wd = m.cfg.learning_rate, m.cfg.weight_decay
    assert isinstance(opt, FlatAdam) and opt.grouped
    assert [g["name"] for g in opt.param_groups] == ["backbone_decay", "backbone_no_decay",
                                                     "rest_decay", "rest_no_decay"]
    assert [g["lr"] for g in opt.param_groups] == [lr * 0.1, lr * 0.1, lr, lr]
    assert opt.wd_dev.cpu().tolist() == [wd, 0.0, wd, 0.0] and opt.flags_dev.cpu().tolist() == [1] * 4
    trainable = [p for p in m.parameters() if p.requires_grad]
    assert len(opt.params) == len(trainable) and all(a is b for a, b in zip(opt.params, trainable))
    names = {id(p): n for n, p in m.named_parameters()}
    before = [p.detach().clone() for p in opt.params]
    d = synthetic.synthetic_batch(1, seed=7)
    data = {k: (v if k in ("intrinsics", "extrinsics") else v.to(DEV)) for k, v in d.items()}
    noise = synthetic.target_noise(1, seed=7).to(DEV)
    m.parking_model._noise = lambda b, device, n: noise
    step = TrainStep(m, data, graph=False, optimizer=opt)
    assert torch.isfinite(step())
    # the first Adam step is lr * g / (|g| + eps) per element, +-lr where |g| >> eps: every
    # group's tensors moved with their own lr and decay; with the other group's they would not
    gmin = torch.stack([p.grad.abs().min() if p.grad is not None else torch.zeros((), device=DEV)
                        for p in opt.params]).cpu().tolist()
    checked = set()
    for k in range(4):  # per group, the tensor whose smallest |g| is largest
        i = max((i for i in range(len(opt.params)) if opt.group_of[i] == k), key=lambda i: gmin[i])
        p, g = opt.params[i], opt.params[i].grad
        if not gmin[i] > 1e-6:
            continue
        checked.add(k)
        glr, gwd = opt.param_groups[k]["lr"], opt.param_groups[k]["weight_decay"]
        g64, p64 = g.double(), before[i].double()
        upd = g64 / (g64.abs() + 1e-8)
        assert float(upd.abs().min()) > 0.99
        want = p64 * (1.0 - glr * gwd) - glr * upd
        other = p64 * (1.0 - glr * gwd) - (lr if glr != lr else lr * 0.1) * upd
        err, err_other = rel_l2(p.detach(), want), rel_l2(p.detach(), other)
        print("full_model", opt.param_groups[k]["name"], names[id(p)], f"{err:.3e} {err_other:.3e}")
        assert err < 1e-6 and err_other > 1e-6, (names[id(p)], err, err_other)
    assert {0, 1} & checked and {2, 3} & checked, checked  # a backbone tensor and another
    bb = [names[id(p)] for p in opt.param_groups[0]["params"] + opt.param_groups[1]["params"]]
    assert bb and all("cam_encoder.backbone." in n for n in bb)
    # checkpoint round trip into a fresh module and optimizer
    sched.step()
    path = os.path.join(tmp_path, "groups.ckpt")
    checkpoint.save_checkpoint(path, m, opt, sched, epoch=1, global_step=1)
    ck = checkpoint.load_checkpoint(path)
    m2 = _full_module()
    out2 = m2.configure_optimizers()
    o2 = out2["optimizer"]
    checkpoint.restore_training(ck, m2, o2, out2["lr_scheduler"])
    for g, h in zip(opt.param_groups, o2.param_groups):
        for key in ("name", "lr", "initial_lr", "weight_decay", "decoupled_weight_decay", "betas", "eps"):
            assert g[key] == h[key], (g["name"], key)
        assert len(g["params"]) == len(h["params"])
    assert opt.param_groups[0]["lr"] != lr * 0.1  # the schedule moved it, and it was restored
    o2.sync_lr()
    opt.sync_lr()
    for t in ("flat", "exp_avg", "exp_avg_sq", "step_count", "stepped", "lr_dev", "wd_dev", "flags_dev"):
        assert torch.equal(getattr(o2, t), getattr(opt, t)), t
