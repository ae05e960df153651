"""KV-cached incremental decoding of the control-token decoder (csrc/ar_decode.hip).

`ControlPredict.predict` (reference model/control_predict.py:60-75) runs the whole decoder
over all T = tf_de_tgt_dim - 1 positions for every generated token and reads one logits row.
The rows before the current position cannot change (the self-attention is causal), the rows
after it are PAD, and the memory's cross-attention K|V is the same in every pass.  Here the
memory K|V is projected once per layer (`start`), each layer keeps its self-attention K/V of
the positions decoded so far, and `step` computes the one new row per sample: six launches per
layer (e2ep_dec_self_attn, e2ep_dec_cross_attn and four e2ep_dec_row_gemv) plus the vocabulary
projection.  The LayerNorms run inside the consumers as they load a row.

`eligible` is the gate of `ControlPredict.predict_tokens`: where it is false the full pass
runs, unchanged.  E2EP_DECODE_CACHE=0 (or `_DECODE_CACHE[0] = False`) switches the path off.
"""
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, nn_ops

# E2EP_DECODE_CACHE=0: predict_tokens always runs the full decoder pass per token (A/B timing:
# scripts/bench_decode_cache.py)
_DECODE_CACHE = [os.environ.get("E2EP_DECODE_CACHE", "1") != "0"]

# launches of the e2ep_dec_* entry points made through this module (tests assert the path
# taken through it)
LAUNCHES = [0]

MAX_BATCH, MAX_T, MAX_MEMORY, MAX_HEAD_DIM, MAX_ROW = 16, 32, 256, 64, 4088


def _call(name, *args):
    LAUNCHES[0] += 1
    _lib.call(name, *args)


def _hooked(mod):
    return bool(mod._forward_hooks or mod._forward_pre_hooks or "forward" in mod.__dict__)


def _plain_norm(norm, E):
    return (isinstance(norm, nn.LayerNorm) and tuple(norm.normalized_shape) == (E,)
            and norm.weight is not None)


def eligible(cp, encoder_out, toks):
    """Whether the incremental path computes `cp.predict_tokens(encoder_out, toks, .)`; see
    the module docstring and DESIGN.md for the list."""
    if not _DECODE_CACHE[0] or cp.training:
        return False
    if not (torch.is_tensor(encoder_out) and encoder_out.is_cuda and encoder_out.dim() == 3
            and encoder_out.dtype == torch.float32 and toks.is_cuda and toks.dtype == torch.long
            and toks.dim() == 2 and toks.shape[0] == encoder_out.shape[0]):
        return False
    if torch.is_grad_enabled() and (encoder_out.requires_grad
                                    or any(p.requires_grad for p in cp.parameters())):
        return False  # autograd would record the call
    B, Sk, E = encoder_out.shape
    T = cp.cfg.tf_de_tgt_dim - 1
    if B > MAX_BATCH or Sk > MAX_MEMORY or not 0 < T <= MAX_T or E > MAX_ROW:
        return False
    if cp.embedding.weight.shape[1] != E or tuple(cp.pos_embed.shape) != (1, T, E):
        return False
    if any(p.dtype != torch.float32 or p.device != encoder_out.device for p in cp.parameters()):
        return False
    if _lib.call_raw("e2ep_gemm_precision", -1) != 0:  # bf16 linears: that mode's full pass stays
        return False
    stack = cp.tf_decoder
    if stack.norm is not None or _hooked(stack):
        return False
    for layer in stack.layers:
        if layer.norm_first or layer.activation is not F.relu or _hooked(layer):
            return False
        if layer.linear1.in_features != E or layer.linear1.out_features > MAX_ROW:
            return False
        if not all(_plain_norm(n, E) for n in (layer.norm1, layer.norm2, layer.norm3)):
            return False
        for att in (layer.self_attn, layer.multihead_attn):
            if _hooked(att) or not att._qkv_same_embed_dim or att.batch_first or \
                    att.bias_k is not None or att.add_zero_attn or att.embed_dim != E:
                return False
            if E % att.num_heads or E // att.num_heads > MAX_HEAD_DIM:
                return False
    return True


class IncrementalDecoder:
    """One decode of a ControlPredict on the current stream: `start(memory)`, then `step(seq,
    t)` for t = 0, 1, ... in order.  Every buffer is allocated in `start`, so start + steps can
    be captured into a HIP graph.  The caller checks `eligible` (an unsupported module or shape
    raises from the entry points: there is no fallback here)."""

    def __init__(self, control_predict):
        self.cp = control_predict
        self.layers = list(control_predict.tf_decoder.layers)

    def start(self, memory):
        """Project the memory (B, Sk, E) to cross-attention K|V once per layer; allocate the
        self-attention caches (layers, B, T, 2, E) and the row buffers."""
        cp = self.cp
        B, Sk, E = memory.shape
        T = cp.cfg.tf_de_tgt_dim - 1
        dev = memory.device
        self.B, self.Sk, self.E, self.T = B, Sk, E, T
        self.V = cp.output.out_features
        with torch.no_grad():
            self.mem_kv = [nn_ops.linear(memory, l.multihead_attn.in_proj_weight[E:],
                                         None if l.multihead_attn.in_proj_bias is None
                                         else l.multihead_attn.in_proj_bias[E:])
                           for l in self.layers]

        def buf(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        self.cache = buf(len(self.layers), B, T, 2, E)
        # x0: the gathered embedding row; att: an attention output; y1..y3: the pre-norm sums
        # ahead of norm1..norm3; h: the FFN hidden row
        self.x0, self.att, self.y1, self.y2, self.y3 = (buf(B, E) for _ in range(5))
        self.h = buf(B, max(l.linear1.out_features for l in self.layers))
        self.logits = buf(B, self.V)
        return self

    def _gemv(self, x, norm, lin, res, res_norm, out, relu=False):
        N, K = lin.weight.shape
        _call("e2ep_dec_row_gemv", _lib.ptr(x), x.stride(0),
              _lib.ptr(norm.weight if norm is not None else None),
              _lib.ptr(norm.bias if norm is not None else None),
              norm.eps if norm is not None else 0.0, _lib.ptr(lin.weight), _lib.ptr(lin.bias),
              _lib.ptr(res), res.stride(0) if res is not None else 0,
              _lib.ptr(res_norm.weight if res_norm is not None else None),
              _lib.ptr(res_norm.bias if res_norm is not None else None),
              res_norm.eps if res_norm is not None else 0.0, _lib.ptr(out), out.stride(0),
              self.B, N, K, int(relu), _lib.stream())

    def step(self, seq, t, logits=True):
        """Decode position t of seq (B, T) int64 (the positions < t were decoded by the steps
        before): fills the caches at t and returns the (B, V) logits of position t (a buffer
        the next step overwrites), or None with logits=False (prefix positions)."""
        cp, B, E, T = self.cp, self.B, self.E, self.T
        s = _lib.stream()
        x, xn = None, None  # the layer's input row (pre-norm) and the norm it still needs
        for li, layer in enumerate(self.layers):
            sa, ca = layer.self_attn, layer.multihead_attn
            H = sa.num_heads
            first = x is None
            _call("e2ep_dec_self_attn", _lib.ptr(x), 0 if first else x.stride(0),
                  _lib.ptr(xn.weight if xn is not None else None),
                  _lib.ptr(xn.bias if xn is not None else None),
                  xn.eps if xn is not None else 0.0, _lib.ptr(cp.embedding.weight),
                  cp.embedding.weight.shape[0], _lib.ptr(cp.pos_embed), _lib.ptr(self.x0),
                  _lib.ptr(seq), seq.stride(0), cp.pad_idx, _lib.ptr(sa.in_proj_weight),
                  _lib.ptr(sa.in_proj_bias), _lib.ptr(self.cache[li]), _lib.ptr(self.att), B, T,
                  int(t), E, H, s)
            if first:
                x = self.x0
            # y1 = out_proj(att) + x;  x1 = norm1(y1)
            self._gemv(self.att, None, sa.out_proj, x, xn, self.y1)
            kv = self.mem_kv[li]
            _call("e2ep_dec_cross_attn", _lib.ptr(self.y1), self.y1.stride(0),
                  _lib.ptr(layer.norm1.weight), _lib.ptr(layer.norm1.bias), layer.norm1.eps,
                  _lib.ptr(ca.in_proj_weight), _lib.ptr(ca.in_proj_bias), _lib.ptr(kv),
                  kv.stride(1), _lib.ptr(self.att), B, self.Sk, E, ca.num_heads, s)
            # y2 = out_proj(att) + x1;  x2 = norm2(y2)
            self._gemv(self.att, None, ca.out_proj, self.y1, layer.norm1, self.y2)
            # h = relu(linear1(x2));  y3 = linear2(h) + x2;  x3 = norm3(y3)
            self._gemv(self.y2, layer.norm2, layer.linear1, None, None, self.h, relu=True)
            self._gemv(self.h, None, layer.linear2, self.y2, layer.norm2, self.y3)
            x, xn = self.y3, layer.norm3
        if not logits:
            return None
        self._gemv(x, xn, cp.output, None, None, self.logits)
        return self.logits


def decode_tokens(cp, encoder_out, toks, steps):
    """`ControlPredict.predict_tokens` on the incremental path (the caller checked `eligible`
    and L + steps <= T): the prefix positions 0 .. L-2 fill the caches, then every step is one
    decoded row, its vocabulary projection and e2ep_token_argmax_append."""
    B, L = toks.shape
    T = cp.cfg.tf_de_tgt_dim - 1
    seq = torch.empty((B, T), dtype=torch.long, device=toks.device)
    _lib.call("e2ep_tokens_init", _lib.ptr(toks), toks.stride(0), B, L, _lib.ptr(seq), T,
              cp.pad_idx, _lib.stream())
    dec = IncrementalDecoder(cp).start(encoder_out)
    for t in range(L - 1):
        dec.step(seq, t, logits=False)
    for i in range(steps):
        length = L + i
        logits = dec.step(seq, length - 1)
        _lib.call("e2ep_token_argmax_append", _lib.ptr(logits), logits.stride(0), B,
                  logits.shape[1], _lib.ptr(seq), T, length, _lib.stream())
    return seq[:, :L + steps]
