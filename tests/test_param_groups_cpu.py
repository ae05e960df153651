"""Parameter groups for FlatAdam, the parts that need no device: the group builder
(optim.parameter_groups), the config keys, the layout-to-torch index mapping and the CPU branch
of configure_optimizers."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def module():
    from tool.config import default_cfg
    from trainer.pl_trainer import ParkingTrainingModule
    torch.manual_seed(0)
    mod = ParkingTrainingModule(default_cfg())
    for p in mod.parking_model.bev_encoder.layer4.parameters():  # as the trainer freezes it
        p.requires_grad_(False)
    return mod


def test_parameter_groups_partition_and_classify(module):
    from e2ep_amd.optim import parameter_groups
    groups, order = parameter_groups(module, 1e-3, 1e-4, backbone_lr_scale=0.1,
                                     no_decay_norm_bias=True, decoupled=True)
    trainable = [p for p in module.parameters() if p.requires_grad]
    assert len(order) == len(trainable) and all(a is b for a, b in zip(order, trainable))
    assert [g["name"] for g in groups] == ["backbone_decay", "backbone_no_decay", "rest_decay",
                                           "rest_no_decay"]
    seen = [id(p) for g in groups for p in g["params"]]
    assert len(seen) == len(set(seen)) and set(seen) == {id(p) for p in trainable}
    frozen = list(module.parking_model.bev_encoder.layer4.parameters())
    assert frozen and not {id(p) for p in frozen} & set(seen)
    by_name = {g["name"]: g for g in groups}
    where = {id(p): g["name"] for g in groups for p in g["params"]}
    for g in groups:
        assert g["decoupled_weight_decay"] is True
        assert g["lr"] == (1e-3 * 0.1 if g["name"].startswith("backbone") else 1e-3)
        assert g["weight_decay"] == (0.0 if g["name"].endswith("no_decay") else 1e-4)
    assert by_name["backbone_decay"]["lr"] == pytest.approx(1e-4)
    named = dict(module.named_parameters())
    mods = dict(module.named_modules())

    def first(pred):
        return next(n for n, p in named.items() if p.requires_grad and pred(n, p))

    def owner(n):
        return mods[n.rsplit(".", 1)[0]]

    bb = "cam_encoder.backbone."
    bn_w = first(lambda n, p: bb not in n and n.endswith(".weight")
                 and isinstance(owner(n), torch.nn.BatchNorm2d))
    conv_w = first(lambda n, p: bb not in n and p.ndim == 4)
    bb_conv = first(lambda n, p: bb in n and p.ndim == 4)
    bb_bias = first(lambda n, p: bb in n and n.endswith(".bias"))
    pos = first(lambda n, p: n.endswith("pos_embed"))
    assert named[pos].ndim > 1  # classified by its name, not by its shape
    assert where[id(named[bn_w])] == "rest_no_decay"
    assert where[id(named[conv_w])] == "rest_decay"
    assert where[id(named[bb_conv])] == "backbone_decay"
    assert where[id(named[bb_bias])] == "backbone_no_decay"
    assert where[id(named[pos])] == "rest_no_decay"
    # one split only
    g2, _ = parameter_groups(module, 1e-3, 1e-4, no_decay_norm_bias=True)
    assert [g["name"] for g in g2] == ["rest_decay", "rest_no_decay"]
    assert id(named[bb_bias]) in {id(p) for p in g2[1]["params"]}  # no backbone split
    g3, _ = parameter_groups(module, 1e-3, 1e-4, backbone_lr_scale=0.5)
    assert [(g["name"], g["lr"]) for g in g3] == [("backbone_decay", 5e-4), ("rest_decay", 1e-3)]


def test_parameter_groups_defaults_are_one_group(module):
    from e2ep_amd.optim import parameter_groups
    groups, order = parameter_groups(module, 1e-3, 1e-4)
    assert len(groups) == 1
    g = groups[0]
    assert (g["lr"], g["weight_decay"], g["decoupled_weight_decay"]) == (1e-3, 1e-4, False)
    assert len(g["params"]) == len(order) and all(a is b for a, b in zip(g["params"], order))
    assert isinstance(g["name"], str)


def test_config_keys_default_off_and_are_typed():
    import yaml
    from tool.config import Configuration, default_cfg, get_cfg
    for cfg in (Configuration(), default_cfg()):
        assert cfg.backbone_lr_scale == 1.0 and isinstance(cfg.backbone_lr_scale, float)
        assert cfg.no_decay_norm_bias is False and cfg.decoupled_weight_decay is False
    with open(os.path.join(ROOT, "e2e-parking-carla_amd", "config", "training.yaml")) as f:
        y = yaml.safe_load(f)
    keys = {"backbone_lr_scale", "no_decay_norm_bias", "decoupled_weight_decay"}
    assert not keys & set(y["parking_model"])
    y["parking_model"].update(backbone_lr_scale="0.1", no_decay_norm_bias=1,
                              decoupled_weight_decay=1)
    cfg = get_cfg(y)
    assert cfg.backbone_lr_scale == 0.1 and isinstance(cfg.backbone_lr_scale, float)
    assert cfg.no_decay_norm_bias is True and cfg.decoupled_weight_decay is True


def test_layout_to_torch_is_the_inverse_of_the_concatenation():
    from e2ep_amd.optim import layout_to_torch
    # layout positions per group: torch numbers the groups concatenated, 3 5 0 | 1 4 | 6 2
    groups = [[3, 5, 0], [1, 4], [6, 2]]
    t = layout_to_torch(groups)
    assert t == [2, 3, 6, 0, 4, 1, 5]
    cat = [i for g in groups for i in g]
    assert [t[i] for i in cat] == list(range(7))
    assert layout_to_torch([[0, 1, 2]]) == [0, 1, 2]
    for bad in ([[0, 1], [1]], [[0, 2]], [[1, 2]]):
        with pytest.raises(ValueError):
            layout_to_torch(bad)


def test_configure_optimizers_cpu_branch_uses_the_same_groups(module):
    from e2ep_amd.optim import parameter_groups
    keys = dict(backbone_lr_scale=0.1, no_decay_norm_bias=True, decoupled_weight_decay=True)
    cfg = module.cfg
    saved = {k: getattr(cfg, k) for k in keys}
    try:
        plain = module.configure_optimizers()["optimizer"]
        assert type(plain) is torch.optim.Adam and len(plain.param_groups) == 1
        assert plain.param_groups[0]["decoupled_weight_decay"] is False
        for k, v in keys.items():
            setattr(cfg, k, v)
        out = module.configure_optimizers()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    opt = out["optimizer"]
    assert type(opt) is torch.optim.Adam
    want, _ = parameter_groups(module, cfg.learning_rate, cfg.weight_decay, 0.1, True, True)
    assert len(opt.param_groups) == len(want) == 4
    for g, w in zip(opt.param_groups, want):
        assert g["name"] == w["name"] and g["lr"] == w["lr"]
        assert g["weight_decay"] == w["weight_decay"] and g["decoupled_weight_decay"] is True
        assert len(g["params"]) == len(w["params"])
        assert all(a is b for a, b in zip(g["params"], w["params"]))
    assert out["lr_scheduler"].optimizer is opt
