"""Configuration bag — same API as the reference's tool/config.py:7-111.

`Configuration` holds the YAML keys as attributes; `get_cfg(yaml_dict)` fills one from the
`parking_model` section.  The device defaults to the HIP device (`cuda` on PyTorch-ROCm).
Optional MI355X keys (absent from reference configs, defaults shown):
  deterministic: False   zero every dropout / drop-connect (SURVEY.md §8c protocol)
  gradient_clip_val: None       global gradient-norm clipping (Lightning's Trainer argument)
  accumulate_grad_batches: 1    micro-batches per optimizer update (Lightning's Trainer argument)
  skip_nonfinite_steps: False   leave out an update whose gradient norm is Inf or NaN
  ema_decay: None               exponential moving average of the weights (0 <= decay < 1)
  ema_warmup: False             timm's warm-up of that decay: min(decay, (1 + n) / (10 + n))
  backbone_lr_scale: 1.0        learning rate of the pretrained cam_encoder.backbone, as a
                                multiple of learning_rate (a parameter group of its own)
  no_decay_norm_bias: False     no weight decay on norm scales, biases (ndim <= 1) and pos_embed
  decoupled_weight_decay: False AdamW's p *= 1 - lr * wd in place of the L2 term
  augment_brightness / augment_contrast / augment_saturation: 0.0   photometric jitter of the
                                training images in the GPU frame decode (needs frame_cache): the
                                factor is uniform on [1 - v, 1 + v], v in [0, 1]
  augment_noise: 0.0            amplitude of uniform per-pixel noise on the [0, 1] image, <= 0.5
  augment_gray_p: 0.0           probability that a frame is turned grey
  augment_per_camera: True      every camera of a sample draws its own jitter
"""
import os
from datetime import datetime

import torch

_KEYS = [
    "log_every_n_steps", "check_val_every_n_epoch", "epochs", "learning_rate", "weight_decay",
    "batch_size", "training_map", "validation_map", "future_frame_nums", "hist_frame_nums",
    "token_nums", "image_crop", "bev_encoder_in_channel", "bev_encoder_out_channel",
    "bev_x_bound", "bev_y_bound", "bev_z_bound", "d_bound", "final_dim", "bev_down_sample",
    "use_depth_distribution", "backbone", "seg_classes", "seg_vehicle_weights", "tf_en_dim",
    "tf_en_heads", "tf_en_layers", "tf_en_dropout", "tf_en_bev_length", "tf_en_motion_length",
    "tf_de_dim", "tf_de_heads", "tf_de_layers", "tf_de_dropout", "tf_de_tgt_dim",
]


class Configuration:
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    data_dir = None
    log_dir = None
    checkpoint_dir = None
    deterministic = False
    gradient_clip_val = None
    accumulate_grad_batches = 1
    skip_nonfinite_steps = False
    ema_decay = None
    ema_warmup = False
    backbone_lr_scale = 1.0
    no_decay_norm_bias = False
    decoupled_weight_decay = False
    augment_brightness = 0.0
    augment_contrast = 0.0
    augment_saturation = 0.0
    augment_noise = 0.0
    augment_gray_p = 0.0
    augment_per_camera = True


for _k in _KEYS:
    setattr(Configuration, _k, None)


def get_cfg(cfg_yaml: dict) -> Configuration:
    section = cfg_yaml["parking_model"]
    cfg = Configuration()
    stamp = datetime.now().strftime("%Y_%-m_%-d_%-H_%-M_%-S")
    cfg.data_dir = section["data_dir"]
    cfg.log_dir = os.path.join(section["log_dir"], "exp_" + stamp)
    cfg.checkpoint_dir = os.path.join(section["checkpoint_dir"], "exp_" + stamp)
    for k in _KEYS:
        setattr(cfg, k, section[k])
    cfg.deterministic = bool(section.get("deterministic", False))
    clip = section.get("gradient_clip_val")
    cfg.gradient_clip_val = None if clip is None else float(clip)
    cfg.accumulate_grad_batches = int(section.get("accumulate_grad_batches", 1))
    cfg.skip_nonfinite_steps = bool(section.get("skip_nonfinite_steps", False))
    ema = section.get("ema_decay")
    cfg.ema_decay = None if ema is None else float(ema)
    cfg.ema_warmup = bool(section.get("ema_warmup", False))
    cfg.backbone_lr_scale = float(section.get("backbone_lr_scale", 1.0))
    cfg.no_decay_norm_bias = bool(section.get("no_decay_norm_bias", False))
    cfg.decoupled_weight_decay = bool(section.get("decoupled_weight_decay", False))
    for k in ("brightness", "contrast", "saturation", "noise", "gray_p"):
        setattr(cfg, "augment_" + k, float(section.get("augment_" + k, 0.0)))
    cfg.augment_per_camera = bool(section.get("augment_per_camera", True))
    return cfg


def default_cfg(**overrides) -> Configuration:
    """The shipped config/training.yaml, with attribute overrides."""
    import yaml

    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "config", "training.yaml")) as f:
        cfg = get_cfg(yaml.safe_load(f))
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg
