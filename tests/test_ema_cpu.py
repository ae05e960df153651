"""Host side of FlatAdam's weight averaging: the two entry points' binding, the config keys and
the checkpoint's "ema" entry (written, read with the restricted unpickler, deployed).  No GPU
call is made."""
import os

import pytest
import torch

from conftest import ROOT
from test_abi_cpu import _codes

ADAM_EMA = ["p", "i", "p", "p", "p", "p", "p", "p", "p", "p", "d", "d", "d", "d", "f", "p", "p", "p",
            "p", "p", "d", "i", "p"]


def test_abi_declares_and_exports_the_entry_points():
    from e2ep_amd import _lib
    sigs = _lib.SIGNATURES
    assert _codes(sigs["e2ep_adam_step_ema"]) == ("i", ADAM_EMA)
    assert _codes(sigs["e2ep_flat_swap"]) == ("i", ["p", "p", "i64", "p"])
    # e2ep_adam_step_clipped's arguments, then ema, ema_updates, ema_decay, ema_warmup, stream
    clipped = _codes(sigs["e2ep_adam_step_clipped"])[1]
    assert ADAM_EMA == clipped[:-1] + ["p", "p", "d", "i"] + clipped[-1:]
    assert len(sigs["e2ep_adam_step"][1]) == 17
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    lib = _lib.load()
    assert hasattr(lib, "e2ep_adam_step_ema") and hasattr(lib, "e2ep_flat_swap")
    assert lib.e2ep_abi_version() == 4  # additive


def test_config_keys_default_off_and_are_typed():
    import yaml
    from tool.config import Configuration, default_cfg, get_cfg
    for cfg in (Configuration(), default_cfg()):
        assert cfg.ema_decay is None and cfg.ema_warmup is False
    with open(os.path.join(ROOT, "e2e-parking-carla_amd", "config", "training.yaml")) as f:
        y = yaml.safe_load(f)
    assert not {"ema_decay", "ema_warmup"} & set(y["parking_model"])
    y["parking_model"].update(ema_decay="0.999", ema_warmup=1)
    cfg = get_cfg(y)
    assert cfg.ema_decay == 0.999 and isinstance(cfg.ema_decay, float)
    assert cfg.ema_warmup is True
    y["parking_model"].update(ema_decay=0)
    cfg = get_cfg(y)
    assert cfg.ema_decay == 0.0 and isinstance(cfg.ema_decay, float)  # 0 is a decay, not "off"


def test_train_step_needs_a_flat_adam_for_ema():
    from e2ep_amd.train import TrainStep
    m = torch.nn.Linear(4, 2)
    m.training_step = lambda batch, idx=0: m(batch["x"]).pow(2).mean()
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    with pytest.raises(ValueError, match="FlatAdam"):
        TrainStep(m, {"x": torch.ones(3, 4)}, graph=False, optimizer=opt, ema_decay=0.9)


@pytest.fixture(scope="module")
def module():
    from tool.config import default_cfg
    from trainer.pl_trainer import ParkingTrainingModule
    torch.manual_seed(0)
    return ParkingTrainingModule(default_cfg())


def _hand_built(module, with_ema=True):
    """A checkpoint dict as checkpoint_dict writes it, its "ema" entry built by hand: every
    parameter + 1 (so it differs from the live value everywhere), every buffer live."""
    from e2ep_amd import checkpoint
    ck = checkpoint.checkpoint_dict(module, epoch=1, global_step=7)
    assert "ema" not in ck  # no optimizer with averaging: the reference's keys only
    if with_ema:
        names = {n for n, _ in module.named_parameters()}
        avg = {k: (v + 1.0 if k in names else v.clone()) for k, v in ck["state_dict"].items()}
        ck["ema"] = {"decay": 0.999, "warmup": True, "num_updates": 12, "state_dict": avg}
    return ck


def test_checkpoint_ema_entry_loads_and_deploys(module, tmp_path):
    from e2ep_amd import checkpoint
    ck = _hand_built(module)
    path = os.path.join(tmp_path, "ema.ckpt")
    torch.save(ck, path)
    back = checkpoint.load_checkpoint(path)  # the restricted unpickler takes the entry
    assert back["ema"]["decay"] == 0.999 and back["ema"]["warmup"] is True
    assert back["ema"]["num_updates"] == 12
    assert list(back["ema"]["state_dict"]) == list(back["state_dict"])
    live = module.parking_model.state_dict()
    params = {n for n, _ in module.parking_model.named_parameters()}
    assert params and len(params) < len(live)
    m = checkpoint.load_parking_model(path, weights="ema")
    for k, v in m.state_dict().items():
        want = live[k] + 1.0 if k in params else live[k]
        assert torch.equal(v, want), k
    assert not m.training
    for m0 in (checkpoint.load_parking_model(path), checkpoint.load_parking_model(path, weights="model")):
        for k, v in m0.state_dict().items():
            assert torch.equal(v, live[k]), k
    with pytest.raises(ValueError, match="weights"):
        checkpoint.load_parking_model(path, weights="average")


def test_checkpoint_without_ema_entry_raises_keyerror(module, tmp_path):
    from e2ep_amd import checkpoint
    path = os.path.join(tmp_path, "plain.ckpt")
    torch.save(_hand_built(module, with_ema=False), path)
    with pytest.raises(KeyError, match="plain.ckpt"):
        checkpoint.load_parking_model(path, weights="ema")
    checkpoint.load_parking_model(path)  # the default still loads


class _AveragingAdam(torch.optim.Adam):
    """torch.optim.Adam with the attributes checkpoint.py reads from a FlatAdam whose weight
    averaging is on (FlatAdam itself needs a HIP device): the average is parameter - 2."""

    def __init__(self, params, **kw):
        super().__init__(params, **kw)
        self.params = self.param_groups[0]["params"]
        self.ema = [p.detach() - 2.0 for p in self.params]
        self.ema_decay, self.ema_warmup = 0.5, False
        self.ema_updates_dev = torch.tensor([3])

    def ema_param(self, i):
        return self.ema[i]


def test_checkpoint_written_with_ema_keeps_adam_format_optimizer_state(module, tmp_path):
    """checkpoint_dict with an averaging optimizer: the "ema" entry holds the average of the
    parameters the optimizer owns and the live value of everything else (here: the frozen
    parameters left out of the optimizer, and the buffers); optimizer_states[0] is still what
    torch.optim.Adam.load_state_dict takes, and carries no average."""
    from e2ep_amd import checkpoint
    named = [(n, p) for n, p in module.named_parameters() if p.requires_grad and p.is_floating_point()]
    owned = named[: len(named) // 2]  # the optimizer owns the first half only
    opt = _AveragingAdam([p for _, p in owned], lr=1e-3)
    for _, p in owned[:3]:
        p.grad = torch.ones_like(p)
    opt.step()
    opt.ema = [p.detach() - 2.0 for p in opt.params]
    path = os.path.join(tmp_path, "avg.ckpt")
    checkpoint.save_checkpoint(path, module, opt, epoch=2, global_step=9)
    ck = checkpoint.load_checkpoint(path)
    e = ck["ema"]
    assert (e["decay"], e["warmup"], e["num_updates"]) == (0.5, False, 3)
    assert type(e["num_updates"]) is int and type(e["decay"]) is float
    own = {n for n, _ in owned}
    for k, v in ck["state_dict"].items():
        assert torch.equal(e["state_dict"][k], v - 2.0 if k in own else v), k
    sd = ck["optimizer_states"][0]
    assert sorted(sd["state"]) == [0, 1, 2]
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    fresh = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for _, p in owned], lr=1e-3)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.state_dict()["state"][0]["exp_avg"], opt.state_dict()["state"][0]["exp_avg"])
