"""Fused flat Adam (csrc/adam.hip) vs torch.optim.Adam (the reference's optimizer,
trainer/pl_trainer.py:116-121), fp32.  The update arithmetic is the same sequence of fp32
operations; contraction choices differ, so parameters agree to ~1e-7 relative."""
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(5,), (64, 3, 3, 3), (4097,), (3, 7), (1, 10, 258), (20000,), (24,)]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(DEV).requires_grad_() for s in SHAPES]


def _grads(step, skip=None):
    g = torch.Generator().manual_seed(100 + step)
    return [None if i == skip else torch.randn(s, generator=g).to(DEV) for i, s in enumerate(SHAPES)]


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_flat_adam_matches_torch_adam(wd):
    from e2ep_amd.optim import FlatAdam
    ref, mine = _params(0), _params(0)
    topt = torch.optim.Adam(ref, lr=1e-3, weight_decay=wd, foreach=False)
    fopt = FlatAdam(mine, lr=1e-3, weight_decay=wd)
    for k in range(6):
        gs = _grads(k)
        for p, q, g in zip(ref, mine, gs):
            p.grad = g.clone()
            q.grad = g.clone()
        topt.step()
        fopt.prepare()
        fopt.step()
    for p, q in zip(ref, mine):
        assert rel_l2(q.detach(), p.detach()) < 1e-6
    # Adam-format state round trip
    sd = fopt.state_dict()
    tsd = topt.state_dict()
    for i in range(len(SHAPES)):
        assert float(sd["state"][i]["step"]) == float(tsd["state"][i]["step"])
        assert rel_l2(sd["state"][i]["exp_avg_sq"], tsd["state"][i]["exp_avg_sq"]) < 1e-6
    f2 = FlatAdam(_params(0), lr=1e-3, weight_decay=wd)
    f2.load_state_dict(tsd)
    assert rel_l2(f2.exp_avg, fopt.exp_avg) < 1e-6


def test_flat_adam_views_and_missing_grad():
    from e2ep_amd.optim import FlatAdam
    ps = _params(1)
    before = [p.detach().clone() for p in ps]
    opt = FlatAdam(ps, lr=1e-2)
    for p, b in zip(ps, before):  # parameters now live in the flat buffer, values unchanged
        assert torch.equal(p.detach(), b)
        assert p.data_ptr() % 16 == 0
    for p, g in zip(ps, _grads(0, skip=2)):
        p.grad = g
    opt.prepare()
    opt.step()
    assert torch.equal(ps[2].detach(), before[2])  # no gradient: not stepped (as torch)
    assert not torch.equal(ps[0].detach(), before[0])
    # torch.optim.Adam keeps no state for a tensor that was never stepped
    ref = _params(1)
    topt = torch.optim.Adam(ref, lr=1e-2)
    for p, g in zip(ref, _grads(0, skip=2)):
        p.grad = g
    topt.step()
    assert sorted(opt.state_dict()["state"]) == sorted(topt.state_dict()["state"]) == [
        i for i in range(len(SHAPES)) if i != 2]


def test_flat_adam_gathered_grads_equal_table_grads():
    """Data-parallel form: gather -> (all-reduce sum of 2 identical ranks) -> scale 1/2."""
    from e2ep_amd.optim import FlatAdam
    a, b = _params(2), _params(2)
    oa, ob = FlatAdam(a, lr=1e-3, weight_decay=1e-4), FlatAdam(b, lr=1e-3, weight_decay=1e-4)
    flat = torch.zeros(ob.numel, device=DEV)
    for k in range(3):
        gs = _grads(k)
        for p, q, g in zip(a, b, gs):
            p.grad, q.grad = g.clone(), g.clone()
        oa.prepare()
        oa.step()
        ob.prepare()
        ob.gather_grads(flat)
        flat.mul_(2.0)  # the all-reduce sum over two ranks with the same gradient
        ob.step(flat, 0.5)
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())


def test_flat_adam_unaligned_gradient_equals_aligned_bitwise():
    """k_adam's scalar path (csrc/adam.hip:53, 83-85): the gradient of the 4097-element tensor
    (a length that is no multiple of 4, two chunks) is a view one float into a larger buffer, so
    it is not 16-byte aligned.  Result: bitwise the aligned run's, and torch.optim.Adam's to 1e-6."""
    from e2ep_amd.optim import FlatAdam
    ref, a, b = _params(3), _params(3), _params(3)
    topt = torch.optim.Adam(ref, lr=1e-3, weight_decay=1e-4, foreach=False)
    oa, ob = FlatAdam(a, lr=1e-3, weight_decay=1e-4), FlatAdam(b, lr=1e-3, weight_decay=1e-4)
    for k in range(3):
        gs = _grads(k)
        for i, (r, p, q, g) in enumerate(zip(ref, a, b, gs)):
            r.grad, p.grad = g.clone(), g.clone()
            if i == 2:
                buf = torch.zeros(g.numel() + 8, device=DEV)
                q.grad = buf[1:1 + g.numel()].copy_(g)
                assert q.grad.data_ptr() % 16 == 4 and p.grad.data_ptr() % 16 == 0
            else:
                q.grad = g.clone()
        topt.step()
        oa.step()
        ob.step()
    for r, p, q in zip(ref, a, b):
        assert torch.equal(p.detach(), q.detach())
        assert rel_l2(q.detach(), r.detach()) < 1e-6
    assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)


def test_flat_adam_zero_and_tiny_gradients():
    """The eps denominator: an all-zero gradient on the first step (0 / eps: nothing moves, as
    torch), then a gradient of 1e-20 (sqrt(v) ~ 3e-22 << eps), then an ordinary one.  Parameters of
    scale 1e-12 make the 1e-20 step visible.  Parameters and exp_avg to 1e-6; exp_avg_sq after
    the 1e-20 step is an fp32 subnormal (1e-43), compared to one subnormal quantum (1.4e-45)."""
    from e2ep_amd.optim import FlatAdam
    shapes = [(5,), (4097,), (3, 7)]
    g = torch.Generator().manual_seed(9)
    init = [torch.randn(s, generator=g) * sc for s, sc in zip(shapes, (1.0, 1e-12, 1.0))]
    ref = [t.clone().to(DEV).requires_grad_() for t in init]
    mine = [t.clone().to(DEV).requires_grad_() for t in init]
    topt = torch.optim.Adam(ref, lr=1e-3, foreach=False)
    fopt = FlatAdam(mine, lr=1e-3)
    for k, fill in enumerate((0.0, 1e-20, None)):
        for p, q in zip(ref, mine):
            gr = torch.randn(p.shape, generator=g).to(DEV) if fill is None else torch.full_like(p, fill)
            p.grad, q.grad = gr.clone(), gr.clone()
        topt.step()
        fopt.step()
        sd, tsd = fopt.state_dict()["state"], topt.state_dict()["state"]
        for i, (p, q) in enumerate(zip(ref, mine)):
            if k == 0:
                assert torch.equal(q.detach().cpu(), init[i])
                assert torch.equal(p.detach().cpu(), init[i])
            assert rel_l2(q.detach(), p.detach()) < 1e-6
            assert rel_l2(sd[i]["exp_avg"], tsd[i]["exp_avg"]) < 1e-6
            assert torch.allclose(sd[i]["exp_avg_sq"], tsd[i]["exp_avg_sq"], rtol=1e-6, atol=1.5e-45)
        if k == 1:
            assert not torch.equal(mine[1].detach().cpu(), init[1])  # the 1e-20 step moved it


def test_flat_adam_follows_learning_rate_changes():
    """The learning rate changed between eager steps through param_groups (what an LR scheduler
    writes): the kernel reads the new value from its device scalar (sync_lr)."""
    from e2ep_amd.optim import FlatAdam
    ref, mine = _params(4), _params(4)
    topt = torch.optim.Adam(ref, lr=1e-3, weight_decay=1e-4, foreach=False)
    fopt = FlatAdam(mine, lr=1e-3, weight_decay=1e-4)
    for k, lr in enumerate((1e-3, 7e-3, 7e-3, 2.5e-5, 0.0)):
        topt.param_groups[0]["lr"] = lr
        fopt.param_groups[0]["lr"] = lr
        for p, q, g in zip(ref, mine, _grads(k)):
            p.grad, q.grad = g.clone(), g.clone()
        before = [q.detach().clone() for q in mine]
        topt.step()
        fopt.step()
        for p, q, b in zip(ref, mine, before):
            assert rel_l2(q.detach(), p.detach()) < 1e-6
            if lr == 0.0:
                assert torch.equal(q.detach(), b)
