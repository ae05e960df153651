"""The train step with its parameter-gradient finishing launches deferred (e2ep_tune key 37 = 2,
the default: e2ep_amd.defer around TrainStep's forward + backward) against the same step with
every launch where it always was (key 37 = 1): the same loss, parameters and gradients, bit
for bit, eager and graph-captured; and a conv weight used twice in one forward."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _module(noise):
    from trainer.pl_trainer import ParkingTrainingModule
    from tool.config import default_cfg
    from weights import make_state
    mod = ParkingTrainingModule(default_cfg(deterministic=True))
    mod.parking_model.load_state_dict(make_state(mod.parking_model.state_dict(), 1234))
    mod = mod.to(DEV).train()
    for p in mod.parking_model.bev_encoder.layer4.parameters():  # as tests/test_train_step_gpu.py
        p.requires_grad_(False)
    mod.parking_model._noise = lambda b, device, n: noise  # fixed target jitter
    return mod


def _batch(b):
    from e2ep_amd import synthetic
    d = synthetic.synthetic_batch(b, seed=7)
    return {k: (v if k in ("intrinsics", "extrinsics") else v.to(DEV)) for k, v in d.items()}


def _two_steps(key37, graph):
    from e2ep_amd import _lib, synthetic
    from e2ep_amd.train import TrainStep
    prev = _lib.load().e2ep_tune(37, key37)
    try:
        mod = _module(synthetic.target_noise(2, seed=7).to(DEV))
        step = TrainStep(mod, _batch(2), graph=graph, warmup=1)
        losses = [step().clone() for _ in range(2)]
        torch.cuda.synchronize()
    finally:
        _lib.load().e2ep_tune(37, prev)
    named = dict(mod.named_parameters())
    return (losses, {k: p.detach().clone() for k, p in named.items()},
            {k: p.grad.clone() for k, p in named.items() if p.grad is not None})


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_train_step_deferred_equals_immediate(graph):
    l2, p2, g2 = _two_steps(2, graph)
    l1, p1, g1 = _two_steps(1, graph)
    assert all(torch.equal(a, b) for a, b in zip(l1, l2)), (l1, l2)
    assert p1.keys() == p2.keys() and g1.keys() == g2.keys() and len(g1) > 100
    for k in g1:
        assert torch.equal(g1[k], g2[k]), "grad " + k
    for k in p1:
        assert torch.equal(p1[k], p2[k]), "param " + k


def _conv_grads(twice, scope):
    """dw of conv(conv(x, w), w) (twice) or conv(x, w) through autograd."""
    from e2ep_amd import _lib, conv, defer
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 64, 16, 16, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(64, 64, 3, 3, generator=g) / 24).to(DEV).requires_grad_(True)
    dy = torch.randn(2, 64, 16, 16, generator=g).to(DEV)

    def fn(k):
        w.grad = x.grad = None
        y = conv.conv2d(x, w, None, (1, 1), (1, 1, 1, 1))
        if twice:
            y = conv.conv2d(y, w, None, (1, 1), (1, 1, 1, 1))
        y.backward(dy * k)
        return _lib.call_raw("e2ep_defer_pending")

    if not scope:
        return fn(1.0), w.grad.clone(), x.grad.clone()
    fn(3.0)  # leaves other values in the allocator's cache (see test_defer_pgrad_gpu.py)
    w.grad = x.grad = None
    with defer.ParamGradDefer():
        pending = fn(1.0)
    return pending, w.grad.clone(), x.grad.clone()


@pytest.mark.parametrize("twice", [False, True], ids=["once", "shared"])
def test_conv_weight_through_autograd(twice):
    """A weight used once defers its slab sum and autograd takes the tensor over as .grad; a
    weight applied twice in the forward takes the immediate path for both gradients (the second
    is added into the first in place)."""
    p0, dw0, dx0 = _conv_grads(twice, False)
    p1, dw1, dx1 = _conv_grads(twice, True)
    assert p0 == 0 and p1 == (0 if twice else 1)
    assert torch.equal(dw0, dw1) and torch.equal(dx0, dx1)
