"""Attention-weights feature, the parts that need no GPU: the model's attention modules are
e2ep_amd.attention.MultiheadAttention without any change to its state dict, initial weights
or RNG stream; e2ep_attn_weights is declared and bound; on CPU tensors the new class is torch's
module."""
import ctypes
import os

import torch
from torch import nn

from helpers import meta


def _cfg():
    from tool.config import default_cfg
    return default_cfg()


def _attn_modules(model):
    return [m for m in model.modules() if isinstance(m, nn.MultiheadAttention)]


def test_model_attention_modules_are_the_new_class():
    from e2ep_amd import attention
    from model.parking_model import ParkingModel
    m = ParkingModel(_cfg())
    mods = _attn_modules(m)
    assert len(mods) == 12  # 4 encoder self_attn + 4 x (decoder self_attn, multihead_attn)
    assert all(type(x) is attention.MultiheadAttention for x in mods)
    enc = m.feature_fusion.tf_encoder.layers
    dec = m.control_predict.tf_decoder.layers
    named = [l.self_attn for l in enc] + [l.self_attn for l in dec] + [l.multihead_attn for l in dec]
    assert {id(x) for x in named} == {id(x) for x in mods}


def test_state_dict_keys_unchanged():
    from model.parking_model import ParkingModel
    sd = ParkingModel(_cfg()).state_dict()
    assert [k for k, _, _ in meta()["state_keys"]] == list(sd.keys())


def test_retargeting_leaves_parameters_and_rng_alone(monkeypatch):
    from e2ep_amd import attention
    from model.feature_fusion import FeatureFusion
    from model.control_predict import ControlPredict
    for cls in (FeatureFusion, ControlPredict):
        torch.manual_seed(11)
        a = cls(_cfg())
        state_a = torch.get_rng_state()
        with monkeypatch.context() as mp:
            mp.setattr(attention, "retarget", lambda stack: stack)  # the step skipped
            torch.manual_seed(11)
            b = cls(_cfg())
            state_b = torch.get_rng_state()
        assert not any(type(x) is attention.MultiheadAttention for x in _attn_modules(b))
        assert all(type(x) is attention.MultiheadAttention for x in _attn_modules(a))
        assert torch.equal(state_a, state_b)
        pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
        assert list(pa) == list(pb)
        for k in pa:
            assert torch.equal(pa[k], pb[k]), k


def test_new_class_adds_no_state():
    from e2ep_amd import attention
    torch.manual_seed(0)
    m = nn.MultiheadAttention(12, 3)
    keys, attrs = list(m.state_dict()), set(vars(m))
    m.__class__ = attention.MultiheadAttention
    assert list(m.state_dict()) == keys and set(vars(m)) == attrs
    assert isinstance(m, nn.MultiheadAttention)


def test_entry_point_declared_and_bound():
    from e2ep_amd import _lib
    assert "e2ep_attn_weights" in _lib.SIGNATURES  # read from include/e2ep.h
    res, args = _lib.SIGNATURES["e2ep_attn_weights"]
    assert res is ctypes.c_int
    assert len(args) == 18  # q, k, lse, 9 ints, scale, causal, key_pad, average, w, stream
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "e2ep_attn_weights")


def test_cpu_tensors_take_the_stock_forward():
    from e2ep_amd import attention
    torch.manual_seed(3)
    stock = nn.MultiheadAttention(12, 3).eval()
    new = nn.MultiheadAttention(12, 3).eval()
    new.load_state_dict(stock.state_dict())
    new.__class__ = attention.MultiheadAttention
    x, mem = torch.randn(5, 2, 12), torch.randn(7, 2, 12)
    kpm = torch.zeros(2, 7, dtype=torch.bool)
    kpm[1, 5:] = True
    with torch.no_grad():
        for kw in ({}, {"average_attn_weights": False}, {"need_weights": False}):
            a = stock(x, mem, mem, key_padding_mask=kpm, **kw)
            b = new(x, mem, mem, key_padding_mask=kpm, **kw)
            assert torch.equal(a[0], b[0])
            assert (a[1] is None and b[1] is None) or torch.equal(a[1], b[1])
