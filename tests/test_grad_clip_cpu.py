"""Host side of gradient clipping / step skipping / accumulation: entry points, config keys,
the Lightning clipping hook and TrainStep's argument check.  No GPU call is made."""
import os
import types

import pytest
import torch

from conftest import ROOT

NEW = ("e2ep_grad_sqnorm", "e2ep_grad_norm_finalize", "e2ep_adam_step_clipped",
       "e2ep_grad_accumulate")


def test_library_exports_the_new_entry_points():
    from e2ep_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    lib = _lib.load()
    for name in NEW:  # the binding is read from include/e2ep.h (argument types: test_abi_cpu.py)
        assert name in _lib.SIGNATURES, f"{name} not declared in include/e2ep.h"
        assert hasattr(lib, name), name
    assert lib.e2ep_abi_version() == 4  # additive: the existing entry points are unchanged
    assert len(_lib.SIGNATURES["e2ep_adam_step"][1]) == 17
    assert len(_lib.SIGNATURES["e2ep_grad_gather"][1]) == 6


def test_config_defaults_are_off():
    from tool.config import Configuration, default_cfg
    for cfg in (Configuration(), default_cfg()):
        assert cfg.gradient_clip_val is None
        assert cfg.accumulate_grad_batches == 1
        assert cfg.skip_nonfinite_steps is False


def test_get_cfg_reads_the_keys():
    import yaml
    from tool.config import get_cfg
    here = os.path.join(ROOT, "e2e-parking-carla_amd", "config", "training.yaml")
    with open(here) as f:
        y = yaml.safe_load(f)
    assert not {"gradient_clip_val", "accumulate_grad_batches",
                "skip_nonfinite_steps"} & set(y["parking_model"])
    y["parking_model"].update(gradient_clip_val=1, accumulate_grad_batches=4,
                              skip_nonfinite_steps=True)
    cfg = get_cfg(y)
    assert cfg.gradient_clip_val == 1.0 and isinstance(cfg.gradient_clip_val, float)
    assert cfg.accumulate_grad_batches == 4 and cfg.skip_nonfinite_steps is True


def _hook_owner():
    from trainer.pl_trainer import ParkingTrainingModule
    return object.__new__(ParkingTrainingModule)  # the hook reads nothing from the module


def test_clipping_hook_sets_flat_adam_attribute():
    """For the fused optimizer the hook only records the value: the clipping happens inside the
    following step, so the gradients are left alone here."""
    mod = _hook_owner()
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.full((4,), 10.0)
    flat = types.SimpleNamespace(max_grad_norm=None, param_groups=[{"params": [p]}])
    mod.configure_gradient_clipping(flat, 0, gradient_clip_val=0.5, gradient_clip_algorithm="norm")
    assert flat.max_grad_norm == 0.5
    mod.configure_gradient_clipping(flat, gradient_clip_val=2, gradient_clip_algorithm=None)
    assert flat.max_grad_norm == 2.0
    assert torch.equal(p.grad, torch.full((4,), 10.0))


def test_clipping_hook_falls_back_to_torch():
    mod = _hook_owner()  # (without Lightning, as this suite runs: torch.nn.utils does the work)
    p = torch.nn.Parameter(torch.ones(4))
    opt = torch.optim.Adam([p], lr=1e-3)
    p.grad = torch.full((4,), 10.0)  # norm 20
    mod.configure_gradient_clipping(opt, gradient_clip_val=1.0, gradient_clip_algorithm="norm")
    assert abs(float(p.grad.norm()) - 1.0) < 1e-5
    p.grad = torch.tensor([10.0, -10.0, 0.1, 0.0])
    mod.configure_gradient_clipping(opt, 0, gradient_clip_val=0.5, gradient_clip_algorithm="value")
    assert torch.equal(p.grad, torch.tensor([0.5, -0.5, 0.1, 0.0]))
    p.grad = torch.full((4,), 10.0)
    mod.configure_gradient_clipping(opt, gradient_clip_val=None)
    assert torch.equal(p.grad, torch.full((4,), 10.0))


@pytest.mark.parametrize("kw", [dict(max_grad_norm=1.0), dict(skip_nonfinite=True),
                                dict(accumulate=2)])
def test_train_step_options_need_flat_adam(kw):
    from e2ep_amd.train import TrainStep
    from test_dist_cpu import _HostSGD, _Tiny, _data
    m = _Tiny()
    params = [p for p in m.parameters() if p.requires_grad]
    with pytest.raises(ValueError):
        TrainStep(m, _data(), graph=False, optimizer=_HostSGD(params, 1e-2), **kw)
    s = TrainStep(m, _data(), graph=False, optimizer=_HostSGD(params, 1e-2))  # defaults: fine
    assert s.accumulate == 1 and s.flat_grad is None
