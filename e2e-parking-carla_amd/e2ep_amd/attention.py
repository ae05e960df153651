"""torch.nn.MultiheadAttention forward on the fused e2ep attention core, with or without the
attention weights.

The reference's transformer layers call `self_attn(x, x, x, ...)` / `multihead_attn(x, mem,
mem)` (torch TransformerEncoderLayer / TransformerDecoderLayer, model/feature_fusion.py:13-14,
model/control_predict.py:19-20).  Here the in-projection stays one e2ep_gemm launch (packed
Q|K|V for self-attention, Q and K|V for cross-attention), the attention core runs as
e2ep_attn_fwd / e2ep_attn_bwd reading Q/K/V in place from that output (no head split
copies, scores never written), and the out-projection is the module's own linear.

`mha(mod, ...)` calls the module itself whenever the fused path would not be the same
computation or would bypass something a caller installed: forward hooks or an
instance-patched forward (the closed-loop agent's attention capture,
agent/parking_agent.py:71-80,266-268), a float attn_mask not declared causal, bias_k /
add_zero_attn, separate projection weights, or shapes outside the kernel's range.

The model's attention modules are `MultiheadAttention` below (model/feature_fusion.py,
model/control_predict.py retarget the class of the modules torch built), whose own forward
runs the same fused path and returns the attention weights from e2ep_attn_weights when asked:
the agent's patch (need_weights=True, average_attn_weights=False) and hook then stay on the
e2ep kernels.  Where autograd records the call, with dropout active, or with a mask the core
does not take, that forward is torch's.
"""
import math
import os

import torch
from torch import nn

from . import _lib, conv, nn_ops, rng, timing

# E2EP_ATTN_SPLIT=1: D first, then dq on the current stream and dk/dv on the side stream.  Off
# by default: the C2 step measured 0.18 ms slower with it (25.58 vs 25.40 ms/step,
# profiles/r02/session6/attn_split_ab.txt) — the two passes contend for the same CUs and the
# extra D launch is on the critical path.
_SPLIT_BWD = os.environ.get("E2EP_ATTN_SPLIT", "0") == "1"

# E2EP_ATTN_WEIGHTS=0: MultiheadAttention.forward always defers to torch's (A/B timing of the
# hooked predict against the stock module: scripts/bench_attn_weights.py)
_FUSED_FORWARD = [os.environ.get("E2EP_ATTN_WEIGHTS", "1") != "0"]

MAX_SEQ = 256
MAX_HEAD_DIM = 64


def _forward(qb, kvb, H, causal, key_pad, p, seed, batch_first):
    """e2ep_attn_fwd on contiguous operands (see _Attn): (o, lse, (packed, dims, E, k_off,
    causal, p)), dims = (B, H, Sq, Sk, dh) and the (sequence, batch) strides of Q, K|V and O."""
    packed = kvb is None
    kvt = qb if packed else kvb
    if batch_first:
        B, Sq, Wq = qb.shape
        _, Sk, Wkv = kvt.shape
    else:
        Sq, B, Wq = qb.shape
        Sk, _, Wkv = kvt.shape
    E = Wq // 3 if packed else Wq
    dh = E // H
    k_off = E if packed else 0
    oshape = (B, Sq, E) if batch_first else (Sq, B, E)
    o = torch.empty(oshape, dtype=qb.dtype, device=qb.device)
    lse = torch.empty(B * H, Sq, dtype=torch.float32, device=qb.device)
    kptr = kvt.data_ptr() + 4 * k_off
    vptr = kptr + 4 * E
    if batch_first:  # (sequence, batch) strides
        dims = (B, H, Sq, Sk, dh, Wq, Sq * Wq, Wkv, Sk * Wkv, E, Sq * E)
    else:
        dims = (B, H, Sq, Sk, dh, B * Wq, Wq, B * Wkv, Wkv, B * E, E)
    with timing.region("attn_fwd"):
        _lib.call("e2ep_attn_fwd", _lib.ptr(qb), kptr, vptr, *dims, 1.0 / math.sqrt(dh),
                  int(causal), _lib.ptr(key_pad), float(p), _lib.ptr(seed), _lib.ptr(o),
                  _lib.ptr(lse), _lib.stream())
    return o, lse, (packed, dims, E, k_off, causal, float(p))


def _weights(qb, kvb, lse, cfg, key_pad, average):
    """e2ep_attn_weights for the forward that returned (lse, cfg): (B, H, Sq, Sk) fp32, or the
    head mean (B, Sq, Sk)."""
    packed, dims, _, k_off, causal, _ = cfg
    B, H, Sq, Sk, dh = dims[:5]
    kvt = qb if packed else kvb
    w = torch.empty((B, Sq, Sk) if average else (B, H, Sq, Sk), dtype=torch.float32,
                    device=qb.device)
    with timing.region("attn_weights"):
        _lib.call("e2ep_attn_weights", _lib.ptr(qb), kvt.data_ptr() + 4 * k_off, _lib.ptr(lse),
                  *dims[:9], 1.0 / math.sqrt(dh), int(causal), _lib.ptr(key_pad), int(average),
                  _lib.ptr(w), _lib.stream())
    return w


class _Attn(torch.autograd.Function):
    """O = dropout_p(softmax(scale Q K^T + mask)) V on (S, B, E)-strided Q/K/V, or (B, S, E)
    with batch_first (the kernels take sequence / batch strides; the dropout counters index
    the logical (b, h, i, j), so both layouts draw the same masks).

    `qb` holds Q at column offset 0 (row stride qb.shape[-1]); `kvb` holds K at column offset
    `k_off` and V at `k_off + E`.  When kvb is None, K/V live in qb itself (packed QKV)."""

    @staticmethod
    def forward(ctx, qb, kvb, H, causal, key_pad, p, seed, batch_first=False):
        o, lse, cfg = _forward(qb, kvb, H, causal, key_pad, p, seed, batch_first)
        ctx.save_for_backward(qb, kvb, o, lse, key_pad, seed)
        ctx.cfg = cfg
        return o

    @staticmethod
    def backward(ctx, do):
        qb, kvb, o, lse, key_pad, seed = ctx.saved_tensors
        packed, dims, E, k_off, causal, p = ctx.cfg
        B, H, Sq = dims[0], dims[1], dims[2]
        kvt = qb if packed else kvb
        do = do.contiguous()
        dqb = torch.empty_like(qb)
        dkvb = None if packed else torch.empty_like(kvb)
        dkvt = dqb if packed else dkvb
        kptr = kvt.data_ptr() + 4 * k_off
        dkptr = dkvt.data_ptr() + 4 * k_off
        ws = torch.empty(_lib.call_raw("e2ep_attn_bwd_workspace", B, H, Sq) // 4,
                         dtype=torch.float32, device=qb.device)
        args = (_lib.ptr(qb), kptr, kptr + 4 * E, _lib.ptr(o), _lib.ptr(do), _lib.ptr(lse), *dims,
                1.0 / math.sqrt(dims[4]), int(causal), _lib.ptr(key_pad), p, _lib.ptr(seed),
                _lib.ptr(dqb), dkptr, dkptr + 4 * E, _lib.ptr(ws))
        with timing.region("attn_bwd"):
            if not (conv.wgrad_overlap() and _SPLIT_BWD):  # serial (A/B, per-kernel timing)
                _lib.call("e2ep_attn_bwd_part", *args, 0, _lib.stream())
            else:
                # D first, then dq here and dk/dv on the side stream concurrently (conv._Fork:
                # every buffer is allocated above, on the current stream)
                _lib.call("e2ep_attn_bwd_part", *args, 1, _lib.stream())
                # dk / dv: ~4 dh-long fma chains per (query, key) pair and head, vector rate
                B_, H_, Sq_, Sk_, dh_ = dims[:5]
                fork = conv._Fork(qb.device, work_us=conv.est_us(
                    8.0 * B_ * H_ * Sq_ * Sk_ * dh_ * 4))
                with fork:
                    _lib.call("e2ep_attn_bwd_part", *args, 3, _lib.stream())
                _lib.call("e2ep_attn_bwd_part", *args, 2, _lib.stream())
                fork.join()
        return dqb, dkvb, None, None, None, None, None, None


def attention(qb, kvb, H, causal=False, key_pad=None, p=0.0, seed=None, batch_first=False,
              need_weights=False, average=True):
    """Functional entry: see _Attn.  key_pad: bool (B, Sk) or None; seed: int32 (1,) device
    tensor, drawn here when p > 0 and none is given; batch_first: (B, S, .) operands and
    output instead of (S, B, .).

    need_weights=True returns (o, w): w the softmax probabilities before dropout, (B, H, Sq, Sk)
    or, with average, their head mean (B, Sq, Sk); masked entries and fully masked rows are 0.
    That call is not recorded by autograd (neither o nor w carries a gradient): it is for
    inference, where MultiheadAttention.forward below uses it."""
    if p > 0.0 and seed is None:
        seed = rng.seed(qb.device)
    qb = qb.contiguous()
    kvb = None if kvb is None else kvb.contiguous()
    if key_pad is not None:
        key_pad = key_pad.contiguous()
        if key_pad.dtype != torch.bool:
            raise TypeError("key_pad must be a bool mask (True = ignore key)")
    if need_weights:
        qb, kvb = qb.detach(), None if kvb is None else kvb.detach()
        o, lse, cfg = _forward(qb, kvb, H, bool(causal), key_pad, float(p), seed, bool(batch_first))
        return o, _weights(qb, kvb, lse, cfg, key_pad, bool(average))
    return _Attn.apply(qb, kvb, H, bool(causal), key_pad, float(p), seed, bool(batch_first))


def _core_fusable(mod, query, key, attn_mask, key_padding_mask, is_causal, batch_first=False):
    """Whether the fused core computes this call of a seq-first module (hooks aside)."""
    if key_padding_mask is not None and key_padding_mask.dtype != torch.bool:
        return False
    if not mod._qkv_same_embed_dim or mod.batch_first or mod.bias_k is not None or mod.add_zero_attn:
        return False
    if attn_mask is not None and not is_causal:
        return False
    if not query.is_cuda or query.dtype != torch.float32 or query.dim() != 3:
        return False
    E, H = mod.embed_dim, mod.num_heads
    sd = 1 if batch_first else 0  # sequence dim
    return (E // H <= MAX_HEAD_DIM and query.shape[sd] <= MAX_SEQ and key.shape[sd] <= MAX_SEQ)


def _fusable(mod, query, key, attn_mask, key_padding_mask, is_causal, batch_first=False):
    if mod._forward_hooks or mod._forward_pre_hooks or "forward" in mod.__dict__:
        return False
    return _core_fusable(mod, query, key, attn_mask, key_padding_mask, is_causal, batch_first)


def mha(mod, query, key, value, attn_mask=None, key_padding_mask=None, is_causal=False,
        skip=False, kv_skip=False, batch_first=False):
    """mod(query, key, value, attn_mask=..., key_padding_mask=..., need_weights=False)[0] for a
    seq-first nn.MultiheadAttention, on the fused core when possible.  `is_causal` asserts
    that attn_mask is the causal (-inf above the diagonal) mask, as torch's is_causal hint.
    skip=True returns (out, query_skip): the layer's residual reads query_skip, whose gradient
    the query projection's input-gradient GEMM accumulates (nn_ops.linear).  kv_skip=True
    (cross attention, key is value) appends key_skip, to be used as the key/value input of the
    next consumer (the next decoder layer's memory).  batch_first: (B, S, E) query / key /
    value and output (the module itself stays seq-first: its fallback call gets transposes)."""
    def ret(out, qs, ks):
        r = (out,) + ((qs,) if skip else ()) + ((ks,) if kv_skip else ())
        return r if len(r) > 1 else out

    def t(z):
        return z.transpose(0, 1) if batch_first else z

    if not _fusable(mod, query, key, attn_mask, key_padding_mask, is_causal, batch_first):
        out = mod(t(query), t(key), t(value), attn_mask=attn_mask,
                  key_padding_mask=key_padding_mask, need_weights=False,
                  is_causal=bool(is_causal) and attn_mask is not None)[0]
        return ret(t(out), query, key)
    E, H = mod.embed_dim, mod.num_heads
    W, bias = mod.in_proj_weight, mod.in_proj_bias
    p = mod.dropout if mod.training else 0.0
    if query is key and key is value:
        qkv, qs = nn_ops.linear(query, W, bias, skip=True)
        ks = qs  # self attention: one input (kv_skip is for cross attention)
        o = attention(qkv, None, H, is_causal, key_padding_mask, p, batch_first=batch_first)
    else:
        if key is not value:
            out = mod(t(query), t(key), t(value), attn_mask=attn_mask,
                      key_padding_mask=key_padding_mask, need_weights=False)[0]
            return ret(t(out), query, key)
        # one Function over the whole in_proj_weight: its backward writes the q and kv row
        # blocks of dW / db in place (a weight split would concatenate them: 2 cat launches)
        q, kv, qs, ks = nn_ops.in_proj_qkv(query, key, W, bias, E)
        o = attention(q, kv, H, is_causal, key_padding_mask, p, batch_first=batch_first)
    out = nn_ops.linear(o, mod.out_proj.weight, mod.out_proj.bias)
    return ret(out, qs, ks)


def _same(a, b):
    """a and b are one tensor, or views of the same elements (mha's fallback call hands the
    module three separate transposed views of one activation)."""
    return a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape
                      and a.stride() == b.stride() and a.dtype == b.dtype)


class MultiheadAttention(nn.MultiheadAttention):
    """nn.MultiheadAttention (no parameter, buffer or state of its own: an existing module
    becomes one by `mod.__class__ = MultiheadAttention`) whose forward runs on the e2ep
    kernels, attention weights included: in-projection (e2ep_gemm), e2ep_attn_fwd,
    e2ep_attn_weights when need_weights, out-projection.  So a caller that patches the module's
    forward to ask for the weights and hooks its output (agent/parking_agent.py:71-91) stays on
    the fused path.

    Taken when the fused core computes the call (_core_fusable: seq-first fp32 HIP operands,
    key is value, no mask beyond key padding and a declared-causal attn_mask), the effective
    dropout is 0 and autograd records nothing (grad mode off, or no operand or parameter
    requires grad); every other call is torch's forward, unchanged.  A fully masked row gives
    zero weights here where torch gives NaN (known difference)."""

    def _fused(self, query, key, value, key_padding_mask, attn_mask, is_causal):
        if not _FUSED_FORWARD[0] or not (torch.is_tensor(key) and torch.is_tensor(value)):
            return False
        if not _core_fusable(self, query, key, attn_mask, key_padding_mask, is_causal):
            return False
        if not _same(key, value) or key.dim() != 3 or key.dtype != query.dtype or not key.is_cuda:
            return False
        if key.shape[1] != query.shape[1] or key.shape[2] != query.shape[2]:
            return False
        if key_padding_mask is not None and tuple(key_padding_mask.shape) != (key.shape[1], key.shape[0]):
            return False
        if attn_mask is not None and tuple(attn_mask.shape) != (query.shape[0], key.shape[0]):
            return False
        if is_causal and attn_mask is None:  # torch rejects the hint without its mask
            return False
        if self.training and self.dropout > 0.0:
            return False
        if torch.is_grad_enabled() and any(
                t is not None and t.requires_grad
                for t in (query, key, value, self.in_proj_weight, self.in_proj_bias,
                          self.out_proj.weight, self.out_proj.bias)):
            return False
        return True

    def forward(self, query, key, value, key_padding_mask=None, need_weights=True, attn_mask=None,
                average_attn_weights=True, is_causal=False):
        if not self._fused(query, key, value, key_padding_mask, attn_mask, is_causal):
            return super().forward(query, key, value, key_padding_mask=key_padding_mask,
                                   need_weights=need_weights, attn_mask=attn_mask,
                                   average_attn_weights=average_attn_weights, is_causal=is_causal)
        # (S, B, E) views of batch-first activations (transformer.encoder runs the stack
        # batch-first): run on the (B, S, E) rows as they lie, no transposed copy.  (With one
        # sample both layouts are the same rows; batch-first keeps the caller's strides.)
        bf = query.transpose(0, 1).is_contiguous() and key.transpose(0, 1).is_contiguous() and \
            not (query.shape[1] > 1 and query.is_contiguous() and key.is_contiguous())
        if bf:
            query, key = query.transpose(0, 1), key.transpose(0, 1)
        H, W, bias = self.num_heads, self.in_proj_weight, self.in_proj_bias
        causal = attn_mask is not None  # _core_fusable: a mask here is the declared causal one
        if _same(query, key):
            q, kv = nn_ops.linear(query, W, bias), None
        else:
            q, kv, _, _ = nn_ops.in_proj_qkv(query, key, W, bias, self.embed_dim)
        if need_weights:
            o, w = attention(q, kv, H, causal, key_padding_mask, batch_first=bf, need_weights=True,
                             average=average_attn_weights)
        else:
            o, w = attention(q, kv, H, causal, key_padding_mask, batch_first=bf), None
        out = nn_ops.linear(o, self.out_proj.weight, self.out_proj.bias)
        return (out.transpose(0, 1) if bf else out), w


def retarget(stack):
    """Make every nn.MultiheadAttention of a transformer stack a MultiheadAttention, in place
    (the class of the module torch built is switched; no module is constructed, so parameters,
    state-dict keys and the RNG stream of the model's constructor are untouched)."""
    for mod in stack.modules():
        if type(mod) is nn.MultiheadAttention:
            mod.__class__ = MultiheadAttention
    return stack
