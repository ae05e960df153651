"""The whole ParkingModel with part of it frozen: the fine-tuning recipes a user of the
reference's API applies (requires_grad_(False) on the camera encoder, the same with the encoder
in eval(), or only the camera encoder trainable).

The B=2 deterministic module of test_model_gpu.py with make_state weights, the same batch and
noise.  Freezing changes no forward value and not the mathematics of the remaining gradients, so
the two train-mode configurations are held to the reference's golden vectors exactly as
test_deterministic_train_step_matches_reference holds the unfrozen model.  The camera encoder
in eval() has no golden: the oracle (oracle/parking_ref.py, plain torch modules with the same
parameter names) is put in the same mode on the CPU in fp32 and fp64 and takes the golden's
place under the same bound.

Frozen parameters receive no gradient in any configuration.  A frozen BatchNorm left in
train() still updates its running statistics (as torch.nn.BatchNorm2d does; requires_grad does
not reach buffers), so "nothing moves" is asserted for the parameters there and for the
buffers of the eval() encoder."""
import functools

import pytest
import torch

from helpers import golden, rel_l2
from test_model_gpu import TOL, _scalar_rel, _within_reference_noise

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAM = "bev_model.cam_encoder."
LOSSES = (("control_loss", "loss_control"), ("segmentation_loss", "loss_seg"), ("depth_loss", "loss_depth"))
# parameters of the never-run bev_encoder.layer4 (reference model/bev_encoder.py:21,23-36)
NEVER_RUN = "bev_encoder.layer4."


def _freeze(model, config):
    """model: the ParkingModel (product or oracle: same module names)."""
    cam = model.bev_model.cam_encoder
    if config in ("cam_frozen", "cam_frozen_eval"):
        cam.requires_grad_(False)
    if config == "cam_frozen_eval":
        cam.eval()
    if config == "only_cam":
        model.requires_grad_(False)
        cam.requires_grad_(True)
    return model


def _module(config, freeze_layer4=False):
    from tool.config import default_cfg
    from trainer.pl_trainer import ParkingTrainingModule
    from weights import make_state
    mod = ParkingTrainingModule(default_cfg(deterministic=True))
    mod.parking_model.load_state_dict(make_state(mod.parking_model.state_dict(), 1234))
    mod = mod.to(DEV).train()
    if freeze_layer4:  # as test_train_step_gpu.py's module
        mod.parking_model.bev_encoder.layer4.requires_grad_(False)
    _freeze(mod.parking_model, config)
    return mod


def _step(config):
    """One eager forward + backward; losses, outputs and gradients on the host."""
    from e2ep_amd import synthetic
    mod = _module(config)
    data = synthetic.synthetic_batch(2, seed=5)
    noise = synthetic.target_noise(2, seed=5).to(DEV)
    losses, outs = mod.compute_losses(data, noise)
    losses["train_loss"].backward()
    torch.cuda.synchronize()
    params = dict(mod.parking_model.named_parameters())
    return dict(losses={k: float(v.detach()) for k, v in losses.items()}, outs=[o.detach().cpu() for o in outs],
                grads={k: (None if p.grad is None else p.grad.cpu()) for k, p in params.items()},
                trainable={k for k, p in params.items() if p.requires_grad})


_eager = functools.lru_cache(maxsize=None)(_step)  # one run per configuration, shared


def _check_none_and_finite(run, full):
    """Frozen parameters have no gradient; trainable ones have one exactly where the unfrozen
    model's have (all but the never-run bev_encoder.layer4), and it is finite."""
    for k, g in run["grads"].items():
        if k not in run["trainable"]:
            assert g is None, f"frozen {k} got a gradient"
            continue
        assert (g is None) == (full["grads"][k] is None), f"trainable {k}: gradient {'missing' if g is None else 'unexpected'}"
        assert (g is None) == k.startswith(NEVER_RUN), k
        assert g is None or torch.isfinite(g).all(), k
    assert all(torch.isfinite(o).all() for o in run["outs"])


def _report_bitwise(config, run, full):
    """Whether the trainable gradients are bitwise the unfrozen run's.  Not asserted: it does
    not hold by construction (a frozen neighbour moves an op from its paired launch to the
    forked one, or off the e2ep_se_bwd_bn route: tests/test_grad_subsets_gpu.py)."""
    from test_model_b8_gpu import _record
    live = [k for k in sorted(run["trainable"]) if run["grads"][k] is not None]
    same = [k for k in live if torch.equal(run["grads"][k], full["grads"][k])]
    worst = max(live, key=lambda k: rel_l2(run["grads"][k], full["grads"][k]))
    e = rel_l2(run["grads"][worst], full["grads"][worst])
    print(f"{config}: {len(same)} of {len(live)} trainable gradients bitwise equal to the unfrozen "
          f"run's; largest rel-L2 difference {e:.3e} ({worst})")
    _record("frozen_model", config, bitwise_equal=len(same), trainable=len(live), worst_rel_l2=e)


@pytest.mark.parametrize("config", ["cam_frozen", "only_cam"])
def test_frozen_train_mode_matches_reference(config):
    from weights import make_grad_probe_keys
    run, full = _eager(config), _eager("unfrozen")
    _check_none_and_finite(run, full)
    assert len(run["trainable"]) < len(full["trainable"])
    frozen_cam = all(k not in run["trainable"] for k in run["grads"] if k.startswith(CAM))
    assert frozen_cam == (config == "cam_frozen")
    # the forward does not depend on who wants a gradient
    assert run["losses"] == full["losses"]
    for a, b in zip(run["outs"], full["outs"]):
        assert torch.equal(a, b)
    g32, g64 = golden("model_train_b2.npz"), golden("model_train_b2_fp64.npz")
    for k, gk in LOSSES:  # test_deterministic_train_step_matches_reference's loss bound
        e_prod, e_ref = _scalar_rel(run["losses"][k], g64[gk]), _scalar_rel(g32[gk], g64[gk])
        assert e_prod <= max(TOL, 2 * e_ref), (k, e_prod, e_ref)
    probes = [k for k in make_grad_probe_keys(run["grads"].keys()) if k in run["trainable"]]
    assert len(probes) >= 5
    for k in probes:
        _within_reference_noise("grad " + k, run["grads"][k].reshape(-1)[:4096], g32["gslice::" + k],
                                g64["gslice::" + k])
    _report_bitwise(config, run, full)


def _make_fp64():
    """tests/golden/make_fp64.py, the module that wrote the fp64 goldens."""
    import importlib.util
    import os
    from helpers import GOLDEN
    spec = importlib.util.spec_from_file_location("make_fp64", os.path.join(GOLDEN, "make_fp64.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _oracle(dtype):
    """The oracle with the camera encoder frozen and in eval(), one train-mode forward +
    backward on the CPU: losses, outputs and gradients.  Built by the goldens' own protocol
    (make_fp64.oracle_model and the batch of its main()): fp64 arithmetic everywhere except the
    pillar geometry — bev_model's frustum / bev_res / bev_start_pos / bev_dim and the batch's
    intrinsics / extrinsics stay fp32, so every point lands in the voxel it lands in in fp32 and
    the fp64 result is the same function's, not another splat's."""
    from e2ep_amd import synthetic
    from oracle import parking_ref as O
    with torch.random.fork_rng():  # oracle_model seeds the global generator
        m = _make_fp64().oracle_model(dtype)
    assert m.bev_model.frustum.dtype == torch.float32
    m = _freeze(m.train(), "cam_frozen_eval")
    data = synthetic.synthetic_batch(2, seed=5)
    data = {k: (v.to(dtype) if v.is_floating_point() and k not in ("intrinsics", "extrinsics") else v)
            for k, v in data.items()}
    losses, outs = O.train_losses(m, data, synthetic.target_noise(2, seed=5))
    losses["train_loss"].backward()
    return ({k: float(v.detach()) for k, v in losses.items()}, [o.detach() for o in outs],
            {k: p.grad for k, p in m.named_parameters()})


def test_frozen_eval_encoder_matches_oracle():
    """requires_grad_(False) + eval() on the camera encoder, the rest training: its BatchNorms
    normalise with their running statistics and its drop-connect is off, so the forward differs
    from the golden's.  Against the oracle in the same mode, with test_model_gpu.py's bound (the
    oracle's own fp32 error against its fp64 result, x2, or 1e-4)."""
    from weights import make_grad_probe_keys
    run, full = _eager("cam_frozen_eval"), _eager("unfrozen")
    _check_none_and_finite(run, full)
    again = _step("cam_frozen_eval")  # run to run
    assert run["losses"] == again["losses"]
    for k, g in run["grads"].items():
        assert (g is None and again["grads"][k] is None) or torch.equal(g, again["grads"][k]), k
    assert run["losses"] != full["losses"]  # the encoder really ran in eval
    l32, o32, g32 = _oracle(torch.float32)
    l64, o64, g64 = _oracle(torch.float64)
    for k, _ in LOSSES:
        e_prod, e_ref = _scalar_rel(run["losses"][k], l64[k]), _scalar_rel(l32[k], l64[k])
        print(f"{k}: product {e_prod:.2e}, oracle fp32 {e_ref:.2e}")
        assert e_prod <= max(TOL, 2 * e_ref), (k, e_prod, e_ref)
    pc, ps, pd = run["outs"]
    _within_reference_noise("pred_control", pc, o32[0], o64[0])
    _within_reference_noise("seg_slice", ps[:, :, 90:110, 90:110], o32[1][:, :, 90:110, 90:110],
                            o64[1][:, :, 90:110, 90:110])
    _within_reference_noise("depth_slice", pd[:, :, 10:14], o32[2][:, :, 10:14], o64[2][:, :, 10:14])
    probes = [k for k in make_grad_probe_keys(run["grads"].keys()) if k in run["trainable"]]
    assert len(probes) >= 5
    for k in probes:
        assert g64[k] is not None, k
        print(f"grad {k}: product {rel_l2(run['grads'][k], g64[k]):.2e}, oracle fp32 {rel_l2(g32[k], g64[k]):.2e}")
        _within_reference_noise("grad " + k, run["grads"][k].reshape(-1)[:4096],
                                g32[k].reshape(-1)[:4096], g64[k].reshape(-1)[:4096])
    for k, g in g64.items():  # the oracle's frozen set is the product's
        assert (g is None) == (run["grads"][k] is None), k


def _batch(b):
    from e2ep_amd import synthetic
    d = synthetic.synthetic_batch(b, seed=7)
    return {k: (v if k in ("intrinsics", "extrinsics") else v.to(DEV)) for k, v in d.items()}


def _train_module(config, noise):
    mod = _module(config, freeze_layer4=True)
    mod.parking_model._noise = lambda b, device, n: noise  # fixed target jitter
    return mod


def _cam_state(mod):
    cam = mod.parking_model.bev_model.cam_encoder
    return ({k: p.detach().clone() for k, p in cam.named_parameters()},
            {k: b.detach().clone() for k, b in cam.named_buffers()})


def test_graph_step_matches_eager_with_frozen_camera_encoder():
    """test_graph_step_matches_eager with the camera encoder frozen (left in train()): the
    captured step replays the eager steps within the same bounds, no frozen parameter moves,
    and the frozen BatchNorms' running statistics — which a train() BatchNorm updates whether
    or not its affine is trainable — agree between the two."""
    from e2ep_amd import synthetic
    from e2ep_amd.train import TrainStep
    noise = synthetic.target_noise(2, seed=7).to(DEV)
    warm = 2
    m_e, m_g = _train_module("cam_frozen", noise), _train_module("cam_frozen", noise)
    p0, b0 = _cam_state(m_e)
    s_e = TrainStep(m_e, _batch(2), graph=False)
    s_g = TrainStep(m_g, _batch(2), graph=True, warmup=warm)  # runs `warm` eager steps
    assert all(p.requires_grad for p in s_g.params) and len(s_g.params) == len(s_e.params)
    for _ in range(warm):
        s_e()
    losses_e = [float(s_e()) for _ in range(2)]
    losses_g = [float(s_g()) for _ in range(2)]
    for a, b in zip(losses_e, losses_g):
        assert abs(a / b - 1) < 1e-6, (losses_e, losses_g)
    assert losses_g[1] != losses_g[0]  # the replayed optimizer step really updates weights
    pe = dict(m_e.named_parameters())
    for k, p in m_g.named_parameters():
        assert rel_l2(p.detach(), pe[k].detach()) < 1e-6, k
    for m in (m_e, m_g):
        p1, b1 = _cam_state(m)
        for k, v in p0.items():
            assert torch.equal(p1[k], v), f"frozen {k} moved"
            assert dict(m.parking_model.bev_model.cam_encoder.named_parameters())[k].grad is None, k
        moved = [k for k, v in b0.items() if not torch.equal(b1[k], v)]
        assert any(k.endswith("running_mean") for k in moved)  # train(): statistics are tracked
    be, bg = _cam_state(m_e)[1], _cam_state(m_g)[1]
    for k, v in be.items():
        if k.endswith("num_batches_tracked"):
            assert torch.equal(v, bg[k]) and int(v) == warm + 2, k
        else:
            assert rel_l2(bg[k], v) < 1e-6, k


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_steps_leave_frozen_eval_encoder_untouched(graph):
    """The usual fine-tuning recipe through TrainStep, eager and captured (warmup=2, then
    replays: a counter or running-statistics update baked into the graph would show here):
    after the steps every parameter and every buffer of the frozen eval() camera encoder —
    running_mean, running_var and num_batches_tracked of each BatchNorm — is bit-identical to
    its initial value, while the rest of the model trains."""
    from e2ep_amd import synthetic
    from e2ep_amd.train import TrainStep
    noise = synthetic.target_noise(2, seed=7).to(DEV)
    mod = _train_module("cam_frozen_eval", noise)
    p0, b0 = _cam_state(mod)
    w0 = mod.parking_model.control_predict.output.weight.detach().clone()
    step = TrainStep(mod, _batch(2), graph=graph, **({"warmup": 2} if graph else {}))
    losses = [float(step()) for _ in range(2)]
    assert all(l == l for l in losses) and losses[0] != losses[1]
    assert not mod.parking_model.bev_model.cam_encoder.training
    p1, b1 = _cam_state(mod)
    for k, v in p0.items():
        assert torch.equal(p1[k], v), f"frozen {k} moved"
    assert any(k.endswith("num_batches_tracked") for k in b0)
    for k, v in b0.items():
        assert torch.equal(b1[k], v), f"buffer {k} of the eval() encoder moved"
    assert not torch.equal(mod.parking_model.control_predict.output.weight.detach(), w0)
    # the BatchNorms outside the encoder are in train(): theirs count every step
    n = int(mod.parking_model.bev_encoder.bn1.num_batches_tracked)
    assert n == (4 if graph else 2), n
