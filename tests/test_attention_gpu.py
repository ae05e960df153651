"""Fused attention core (e2ep_attn_fwd / e2ep_attn_bwd) vs torch.nn.MultiheadAttention.

Shapes are the reference's transformer calls (model/feature_fusion.py:13-14: self-attention
over 256 BEV tokens; model/control_predict.py:19-20: causal + key-padding self-attention over
14 control tokens and cross-attention to the 256-token memory), d_model 258, 6 heads.
Reference = the same module in fp64 on the CPU; tolerance rel-L2 <= 1e-4 (north_star) on the
output and on every gradient.  Dropout is checked against an fp64 restatement that applies
the kernel's own keep mask (e2ep_attn_keep_mask), so the mask is the only shared piece."""
import math

import pytest
import torch
from torch import nn

from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, H = 258, 6


def _module(seed):
    torch.manual_seed(seed)
    m = nn.MultiheadAttention(E, H, dropout=0.0)
    with torch.no_grad():
        m.in_proj_bias.normal_(0, 0.1)
        m.out_proj.bias.normal_(0, 0.1)
    return m


def _grads(m, *xs):
    return [x.grad for x in xs] + [m.in_proj_weight.grad, m.in_proj_bias.grad,
                                   m.out_proj.weight.grad, m.out_proj.bias.grad]


@pytest.mark.parametrize("case", ["enc_self", "dec_self", "dec_cross", "ragged", "tiny_cross",
                                  "dec_self_17"])
def test_mha_matches_module(case):
    from e2ep_amd import attention
    g = torch.Generator().manual_seed(7)
    B = 8
    Sq, Sk = {"enc_self": (256, 256), "dec_self": (14, 14), "dec_cross": (14, 256),
              "ragged": (77, 130), "tiny_cross": (5, 9), "dec_self_17": (17, 17)}[case]
    m = _module(len(case))
    m64 = _module(len(case)).double()
    x = torch.randn(Sq, B, E, generator=g)
    mem = torch.randn(Sk, B, E, generator=g)
    dy = torch.randn(Sq, B, E, generator=g)
    causal = case.startswith("dec_self")
    kpm = None
    mask = None
    if causal:
        kpm = torch.zeros(B, Sk, dtype=torch.bool)
        for b in range(B):
            kpm[b, Sk - b:] = True  # sample b has b PAD tokens at the end
        mask = torch.full((Sk, Sk), float("-inf")).triu(1)
    self_attn = case in ("enc_self", "dec_self", "dec_self_17")
    # reference (fp64, CPU)
    xr = x.double().requires_grad_(True)
    mr = xr if self_attn else mem.double().requires_grad_(True)
    yr = m64(xr, mr, mr, attn_mask=None if mask is None else mask.double(), key_padding_mask=kpm,
             need_weights=False)[0]
    (yr * dy.double()).sum().backward()
    # fused path
    md = m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    memd = xd if self_attn else mem.to(DEV).requires_grad_(True)
    yd = attention.mha(md, xd, memd, memd, attn_mask=None if mask is None else mask.to(DEV),
                       key_padding_mask=None if kpm is None else kpm.to(DEV), is_causal=causal)
    (yd * dy.to(DEV)).sum().backward()
    assert rel_l2(yd.detach().cpu(), yr) < 1e-4
    ins = (xd,) if self_attn else (xd, memd)
    ins_r = (xr,) if self_attn else (xr, mr)
    for a, b in zip(_grads(md, *ins), _grads(m64, *ins_r)):
        assert rel_l2(a.cpu(), b) < 1e-4


def _ref_core(q, k, v, keep, p, causal, kpm):
    """fp64 restatement: (B*H, S, dh) operands, keep mask [BH][Sq][Sk]."""
    s = q @ k.transpose(1, 2) / math.sqrt(q.shape[-1])
    BH, Sq, Sk = s.shape
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool).triu(1), float("-inf"))
    if kpm is not None:
        s = s.masked_fill(kpm.repeat_interleave(BH // kpm.shape[0], 0)[:, None, :], float("-inf"))
    P = torch.softmax(s, -1).nan_to_num(0.0)
    return (P * keep / (1 - p)) @ v


@pytest.mark.parametrize("Sq,Sk,causal", [(256, 256, False), (14, 14, True), (14, 256, False),
                                                (16, 16, True), (17, 9, False)])
def test_attention_dropout_matches_masked_reference(Sq, Sk, causal):
    _dropout_case(Sq, Sk, causal)


# (head dim, S, e2ep_tune key 20, split backward): the vector-kernel instantiations no test
# above launches.  k_attn_fwd / k_attn_bwd_q / k_attn_bwd_kv<DHP, LANES>: <44, 2> (dh 43, key 20 =
# 2), <64, 1> (dh 64 at 17 > 16 tokens), <64, 2>, <64, 4> (14 tokens); k_attn_bwd_d<64> (the
# split backward's D pass, which also runs dq and dk / dv as parts 2 and 3).
@pytest.mark.parametrize("dh,S,lanes,split", [(43, 17, 2, False), (64, 17, 1, False), (64, 17, 2, False),
                                              (64, 14, 1, False), (64, 17, 1, True)])
def test_attention_vector_kernel_variants(dh, S, lanes, split):
    from e2ep_amd import _lib, attention, conv
    old = _lib.call_raw("e2ep_tune", 20, lanes)
    split0, attention._SPLIT_BWD = attention._SPLIT_BWD, split
    prev, prev_us = conv.set_wgrad_overlap(split), conv.set_fork_min_us(0)
    try:
        _dropout_case(S, S, False, B=2, dh=dh)
    finally:
        conv.set_wgrad_overlap(prev)
        conv.set_fork_min_us(prev_us)
        attention._SPLIT_BWD = split0
        _lib.call_raw("e2ep_tune", 20, old)
    assert _lib.call_raw("e2ep_tune", 20, 0) == old


def _dropout_case(Sq, Sk, causal, B=4, dh=43):
    from e2ep_amd import _lib, attention
    g = torch.Generator().manual_seed(11)
    p = 0.1
    Ed = H * dh
    qb = torch.randn(Sq, B, Ed, generator=g)
    kvb = torch.randn(Sk, B, 2 * Ed, generator=g)
    do = torch.randn(Sq, B, Ed, generator=g)
    kpm = torch.zeros(B, Sk, dtype=torch.bool)
    kpm[1, Sk - 3:] = True
    seed = torch.tensor([12345], dtype=torch.int32, device=DEV)
    keep = torch.empty(B * H, Sq, Sk, dtype=torch.uint8, device=DEV)
    _lib.call("e2ep_attn_keep_mask", _lib.ptr(seed), B * H, Sq, Sk, p, _lib.ptr(keep), _lib.stream())
    keep = keep.cpu().double()
    assert abs(float(keep.mean()) - (1 - p)) < 0.01
    qd = qb.to(DEV).requires_grad_(True)
    kvd = kvb.to(DEV).requires_grad_(True)
    o = attention.attention(qd, kvd, H, causal, kpm.to(DEV), p, seed)
    (o * do.to(DEV)).sum().backward()

    def heads(t):  # (S, B, H*dh) -> (B*H, S, dh)
        S = t.shape[0]
        return t.reshape(S, B, H, dh).permute(1, 2, 0, 3).reshape(B * H, S, dh)
    qr = qb.double().requires_grad_(True)
    kvr = kvb.double().requires_grad_(True)
    orr = _ref_core(heads(qr), heads(kvr[..., :Ed]), heads(kvr[..., Ed:]), keep, p, causal, kpm)
    orr = orr.reshape(B, H, Sq, dh).permute(2, 0, 1, 3).reshape(Sq, B, Ed)
    (orr * do.double()).sum().backward()
    assert rel_l2(o.detach().cpu(), orr) < 1e-4
    assert rel_l2(qd.grad.cpu(), qr.grad) < 1e-4
    assert rel_l2(kvd.grad.cpu(), kvr.grad) < 1e-4
    # same seed -> same result (the backward regenerates the forward's mask)
    o2 = attention.attention(qd.detach(), kvd.detach(), H, causal, kpm.to(DEV), p, seed)
    assert torch.equal(o2, o.detach())


def test_fully_masked_rows_are_zero():
    from e2ep_amd import attention
    B, S, dh = 2, 20, 43
    qb = torch.randn(S, B, 3 * H * dh, device=DEV, requires_grad=True)
    kpm = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    kpm[1] = True
    o = attention.attention(qb, None, H, False, kpm)
    assert torch.all(o[:, 1] == 0) and torch.isfinite(o).all()
    o.sum().backward()
    assert torch.isfinite(qb.grad).all()


def test_hooked_module_falls_back():
    """A forward hook (the agent's attention capture) must see the module's own call."""
    from e2ep_amd import attention
    m = _module(0).to(DEV)
    seen = []
    h = m.register_forward_hook(lambda mod, args, out: seen.append(out))
    x = torch.randn(16, 2, E, device=DEV)
    y = attention.mha(m, x, x, x)
    h.remove()
    assert len(seen) == 1
    assert rel_l2(y.cpu(), attention.mha(m, x, x, x).cpu()) < 1e-5


def test_graph_replay_draws_new_masks():
    """Under HIP-graph replay the seed tensor is redrawn each replay (torch's graph-safe RNG),
    so consecutive replays use different dropout masks."""
    from e2ep_amd import attention
    qb = torch.randn(64, 2, 3 * E, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        attention.attention(qb, None, H, p=0.1)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = attention.attention(qb, None, H, p=0.1)
    gr.replay()
    a = out.clone()
    gr.replay()
    assert not torch.equal(a, out)


@pytest.mark.parametrize("rows,cin,cout", [(2048, 258, 2048), (2048, 2048, 258), (112, 258, 774),
                                           (3, 5, 7), (1000, 64, 130)])
def test_linear_bias_grad(rows, cin, cout):
    """nn_ops.linear (e2ep_col_sum bias gradient) vs F.linear in fp64."""
    from e2ep_amd import nn_ops
    g = torch.Generator().manual_seed(rows + cout)
    x = torch.randn(rows, cin, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g)
    dy = torch.randn(rows, cout, generator=g)
    ref = [t.double().requires_grad_(True) for t in (x, w, b)]
    (torch.nn.functional.linear(*ref) * dy.double()).sum().backward()
    dev = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
    y = nn_ops.linear(*dev)
    (y * dy.to(DEV)).sum().backward()
    for a, r in zip(dev, ref):
        assert rel_l2(a.grad.cpu(), r.grad) < 1e-5


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_relu_dropout_matches_masked_reference(p):
    """Feed-forward dropout(relu(x)) vs fp64 with the kernel's own keep mask (same hash as the
    attention dropout: counters 0..n-1)."""
    from e2ep_amd import _lib, nn_ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2048, 2048, generator=g)
    dy = torch.randn(2048, 2048, generator=g)
    seed = torch.tensor([777], dtype=torch.int32, device=DEV)
    n = x.numel()
    keep = torch.empty(n, dtype=torch.uint8, device=DEV)
    _lib.call("e2ep_attn_keep_mask", _lib.ptr(seed), 1, 1, n, p, _lib.ptr(keep), _lib.stream())
    keep = keep.cpu().double().view_as(x)
    if p > 0:
        assert abs(float(keep.mean()) - (1 - p)) < 0.002
    xd = x.to(DEV).requires_grad_(True)
    y = nn_ops.relu_dropout(xd, p, seed if p > 0 else None)
    (y * dy.to(DEV)).sum().backward()
    xr = x.double().requires_grad_(True)
    yr = torch.relu(xr) * keep / (1 - p)
    (yr * dy.double()).sum().backward()
    assert rel_l2(y.detach().cpu(), yr) < 1e-6
    assert rel_l2(xd.grad.cpu(), xr.grad) < 1e-6


def test_linear_skip_gradient_accumulated_in_gemm():
    """nn_ops.linear(skip=True): the residual's gradient joins dx inside the addmm."""
    from e2ep_amd import nn_ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(256, 8, 258, generator=g).transpose(0, 1)  # non-contiguous, like the encoder
    w = torch.randn(774, 258, generator=g) / 16
    b = torch.randn(774, generator=g)
    gy = torch.randn(8, 256, 774, generator=g)
    gs = torch.randn(8, 256, 258, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y, xs = nn_ops.linear(xd, w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True), skip=True)
    ((y * gy.to(DEV)).sum() + (xs * gs.to(DEV)).sum()).backward()
    ref = gy.double() @ w.double() + gs.double()
    assert rel_l2(xd.grad.cpu(), ref) < 1e-5


@pytest.mark.parametrize("packed,causal,p", [(True, False, 0.1), (False, False, 0.0), (True, True, 0.1)])
def test_split_backward_equals_serial(packed, causal, p):
    """Backward as D, then dq and dk/dv forked onto two streams (E2EP_ATTN_SPLIT=1) gives bitwise the
    serial e2ep_attn_bwd result, for self-attention (packed QKV: dq and dk/dv written into
    one tensor by the two streams) and cross-attention, with dropout and a causal mask."""
    from e2ep_amd import attention, conv
    attention._SPLIT_BWD, split0 = True, attention._SPLIT_BWD
    torch.manual_seed(5)
    S, Sk, B, dh = 14, 256, 4, 43
    qb = torch.randn(S, B, (3 if packed else 1) * H * dh, device=DEV, requires_grad=True)
    kvb = None if packed else torch.randn(Sk, B, 2 * H * dh, device=DEV, requires_grad=True)
    seed = torch.tensor([1234], dtype=torch.int32, device=DEV)
    g = torch.randn(S, B, H * dh, device=DEV)
    res = []
    for on in (False, True):
        prev = conv.set_wgrad_overlap(on)
        prev_us = conv.set_fork_min_us(0)  # fork at this size too
        try:
            for t in (qb, kvb):
                if t is not None:
                    t.grad = None
            o = attention.attention(qb, kvb, H, causal and packed, None, p, seed)
            o.backward(g)
            res.append([t.grad.clone() for t in (qb, kvb) if t is not None])
        finally:
            conv.set_wgrad_overlap(prev)
            conv.set_fork_min_us(prev_us)
    attention._SPLIT_BWD = split0
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_fully_masked_row_fused_zero_module_nan():
    """Documented difference: a query whose keys are all padding gives 0 from the
    fused path (output = the out-projection bias) where torch's MultiheadAttention (the
    fallback / reference path) gives NaN on its math path; rows with any live key agree.  The
    reference's decoder never builds such a row."""
    from e2ep_amd import attention
    m = _module(3).to(DEV).train()  # training-mode math path in torch (no fast path)
    x = torch.randn(12, 2, E, device=DEV)
    kpm = torch.zeros(2, 12, dtype=torch.bool, device=DEV)
    kpm[1] = True
    with torch.no_grad():
        fused = attention.mha(m, x, x, x, key_padding_mask=kpm)
        ref = m(x, x, x, key_padding_mask=kpm, need_weights=False)[0]
    # torch's math path gives NaN; an SDPA backend may give the attention-free row instead
    assert torch.isnan(ref[:, 1]).all() or rel_l2(ref[:, 1], fused[:, 1]) < 1e-5
    attn_part = fused[:, 1] - m.out_proj.bias  # all-masked rows: attention output 0
    assert torch.isfinite(fused).all() and attn_part.abs().max() < 1e-6
    assert rel_l2(fused[:, 0], ref[:, 0]) < 1e-5


@pytest.mark.parametrize("Sq,Sk", [(256, 256), (128, 256), (256, 128), (128, 128)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_matrix_core_matches_reference(Sq, Sk, p):
    """The matrix-core kernels (csrc/attn_mf.hip: unmasked, Sq / Sk in {128, 256}, the fusion
    encoder's shape) vs the fp64 restatement with the kernel's own keep mask, and vs the
    vector-FMA kernels (e2ep_tune key 21 = 1) on the same inputs and mask."""
    from e2ep_amd import _lib, attention
    g = torch.Generator().manual_seed(13 + Sq + Sk)
    B, dh = 4, 43
    Ed = H * dh
    qb = torch.randn(Sq, B, Ed, generator=g)
    kvb = torch.randn(Sk, B, 2 * Ed, generator=g)
    do = torch.randn(Sq, B, Ed, generator=g)
    seed = torch.tensor([777], dtype=torch.int32, device=DEV)
    keep = torch.empty(B * H, Sq, Sk, dtype=torch.uint8, device=DEV)
    _lib.call("e2ep_attn_keep_mask", _lib.ptr(seed), B * H, Sq, Sk, p if p > 0 else 0.0,
              _lib.ptr(keep), _lib.stream())
    keep = keep.cpu().double() if p > 0 else torch.ones(B * H, Sq, Sk, dtype=torch.float64)
    outs = {}
    for mf in (3, 2, 1):  # all three passes / forward + dq / none on the matrix cores
        old = _lib.call_raw("e2ep_tune", 21, mf)
        try:
            qd = qb.to(DEV).requires_grad_(True)
            kvd = kvb.to(DEV).requires_grad_(True)
            o = attention.attention(qd, kvd, H, False, None, p, seed if p > 0 else None)
            (o * do.to(DEV)).sum().backward()
        finally:
            _lib.call_raw("e2ep_tune", 21, old)
        outs[mf] = (o.detach().cpu(), qd.grad.cpu(), kvd.grad.cpu())

    def heads(t):
        S = t.shape[0]
        return t.reshape(S, B, H, dh).permute(1, 2, 0, 3).reshape(B * H, S, dh)
    qr = qb.double().requires_grad_(True)
    kvr = kvb.double().requires_grad_(True)
    orr = _ref_core(heads(qr), heads(kvr[..., :Ed]), heads(kvr[..., Ed:]), keep, p, False, None)
    orr = orr.reshape(B, H, Sq, dh).permute(2, 0, 1, 3).reshape(Sq, B, Ed)
    (orr * do.double()).sum().backward()
    for mf in (3, 2):
        for got, ref in zip(outs[mf], (orr.detach(), qr.grad, kvr.grad)):
            assert rel_l2(got, ref) < 1e-5
        for a, b in zip(outs[mf], outs[1]):  # both kernel families, same mask
            assert rel_l2(a, b) < 1e-5
