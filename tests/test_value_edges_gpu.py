"""Kernels on non-finite, saturated, offset and degenerate VALUES (the rest of the suite varies
shapes, tiles and launch paths but draws nearly every input from randn).

Each test compares a kernel with a plain reference of the same operation: torch on the CPU in
fp64, or the oracle's restatement of the reference losses.

Bounds.  Tokens, pooled values, where NaN lands, which tap gets a gradient and "exactly zero"
losses / gradients are compared exactly.  Finite values use the bound the neighbouring test
of the same op applies (rel-L2, helpers.rel_l2).  Inputs with large offsets make fp32 itself
miss some of those bounds; there the rule is `_bound`: when torch's own fp32 CPU op on the
identical input misses the base bound against fp64, the bound is 4 x torch-fp32's error,
computed at run time (4 covers a different but equally valid summation tree; the failures these
inputs target, such as an fp32 one-pass variance, sit at >= 50 x: see
test_offset_inputs_separate_one_pass_variance_from_fp32, which runs on the CPU).  Every such
comparison prints the kernel's error, torch-fp32's error and the bound."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from helpers import rel_l2
from test_nn_ops_gpu import bn_path, se_bn_sums  # noqa: F401  (fixtures)

gpu = pytest.mark.gpu
DEV = "cuda"
EPS, MOM = 1e-3, 0.01  # efficientnet-pytorch's BatchNorm settings
NAN, INF = float("nan"), float("inf")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bound(base, err32):
    """The base bound, or 4 x torch-fp32's own error where that misses the base bound."""
    return base if err32 <= base else 4.0 * err32


def _check(tag, got, ref64, ref32, base):
    e, e32 = rel_l2(got, ref64), rel_l2(ref32, ref64)
    b = _bound(base, e32)
    print(f"{tag}: kernel {e:.3e}, torch fp32 {e32:.3e}, bound {b:.3e}")
    assert e < b, f"{tag}: kernel {e:.3e} vs bound {b:.3e} (torch fp32 {e32:.3e})"


def _same_with_nan(got, ref):
    """Exact equality where NaN == NaN: the NaN positions agree, every other value is bitwise."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    gn, rn = torch.isnan(got), torch.isnan(ref)
    return torch.equal(gn, rn) and torch.equal(got[~gn], ref[~rn])


# ------------------------------------------------------------------------------------------
# 1. token argmax: rows whose softmax is all NaN, ties, saturation
# ------------------------------------------------------------------------------------------
def _argmax_row(kind, V, g):
    r = torch.randn(V, generator=g) * 3
    if kind == "one_nan":
        r[2 * V // 3 + 1] = NAN            # V = 204: index 137, third wave
    elif kind == "two_nan":
        r[V // 4 + 1] = r[V - 1] = NAN     # two lanes / two waves
    elif kind == "one_inf":
        r[V // 2] = INF
    elif kind == "two_inf":
        r[2] = r[V - 2] = INF
    elif kind == "all_neg_inf":
        r[:] = -INF
    elif kind == "two_maxima":
        r[:] = -INF
        r[V // 3] = r[2 * V // 3] = 1.5
    elif kind == "huge":
        r = torch.where(r > 0, torch.tensor(3e38), torch.tensor(-3e38))
        r[0], r[V // 3], r[V - 1] = -3e38, 3e38, 3e38
    else:
        assert kind == "all_equal"
        r[:] = 0.7
    return r


ARGMAX_KINDS = ["one_nan", "two_nan", "one_inf", "two_inf", "all_neg_inf", "two_maxima", "huge",
                "all_equal"]


@gpu
@pytest.mark.parametrize("B,V", [(6, 204), (3, 7)])
def test_token_argmax_append_non_finite_rows(B, V):
    """k_token_argmax_append (csrc/tokens.hip) on rows whose probabilities are all NaN (a NaN, a
    +inf, only -inf: torch.argmax gives 0), rows of -inf with two equal maxima, +-3e38 and
    all-equal rows; one kind per batch element, every kind at both vocabulary sizes.  The token
    is torch.softmax(row).argmax(), lies in [0, V), and no other column changes.  Only the
    append kernel runs: the buffer is never embedded."""
    from e2ep_amd import _lib
    g = _g(B * V)
    T, L = 14, 2
    steps = -(-len(ARGMAX_KINDS) // B)
    seq = torch.full((B, T), -5, dtype=torch.long, device=DEV)
    want = seq.cpu().clone()
    s = _lib.stream()
    for j in range(steps):
        kinds = [ARGMAX_KINDS[(b + j * B) % len(ARGMAX_KINDS)] for b in range(B)]
        rows = torch.stack([_argmax_row(k, V, g) for k in kinds])
        expect = torch.softmax(rows, dim=-1).argmax(dim=-1)
        for k, e in zip(kinds, expect.tolist()):
            if k in ARGMAX_KINDS[:5]:
                assert e == 0, k            # all-NaN probabilities: torch returns index 0
            if k == "two_maxima":
                assert e == V // 3          # the first of the two
        rd = rows.to(DEV)
        _lib.call("e2ep_token_argmax_append", _lib.ptr(rd), rd.stride(0), B, V, _lib.ptr(seq), T,
                  L + j, s)
        want[:, L + j] = expect
        got = seq.cpu()
        assert bool(((got[:, L + j] >= 0) & (got[:, L + j] < V)).all()), (kinds, got[:, L + j])
        assert torch.equal(got, want), (kinds, got[:, L + j].tolist(), expect.tolist())


# ------------------------------------------------------------------------------------------
# 2. max-pool 3x3/2: ties, NaN, -inf
# ------------------------------------------------------------------------------------------
def _maxpool_input(shape, kind):
    N, C, H, W = shape
    g = _g(sum(shape) + len(kind))
    if kind == "ties":
        return torch.randint(0, 3, shape, generator=g).float()
    x = torch.randn(*shape, generator=g)
    if kind == "nan_inf":
        if H > 1:
            x[-1, -1, H - 1, :] = -INF      # one full row of -inf
        x[0, 0, 0, 0] = NAN
        if W > 1:
            x[0, 0, 0, 1] = NAN             # two NaNs inside output (0, 0)'s window
        if H > 2 and W > 2:
            x[-1, 0, 2, W - 1] = NAN
    else:
        assert kind == "neg_inf_plane"
        x[0, 0] = -INF
    return x


@gpu
@pytest.mark.parametrize("kind", ["ties", "nan_inf", "neg_inf_plane"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 2, 3), (1, 5, 5, 4), (3, 2, 7, 64)])
def test_maxpool_ties_nan_inf(shape, kind):
    """k_maxpool_fwd's "NaN wins / first maximum / all -inf window" (csrc/pool.hip:22-37): the
    output equals F.max_pool2d exactly (NaN positions included) and the input gradient, which
    pins the tap that received each gradient, matches fp64."""
    from e2ep_amd import nn_ops
    x = _maxpool_input(shape, kind)
    xd = x.to(DEV).requires_grad_(True)
    y = nn_ops.max_pool3s2(xd)
    dy = torch.randn(y.shape, generator=_g(1))
    y.backward(dy.to(DEV))
    x64 = x.double().requires_grad_(True)
    y64 = F.max_pool2d(x64, 3, 2, 1)
    y64.backward(dy.double())
    assert y.shape == y64.shape and _same_with_nan(y, y64)
    assert rel_l2(xd.grad, x64.grad) < 1e-7


# ------------------------------------------------------------------------------------------
# 3. global average pool and SE gate: wave-stride remainders, saturated gates, offset planes
# ------------------------------------------------------------------------------------------
GATES = [0.3, 20.0, -20.0, 100.0, -100.0, -1.2, 2.5]
HW_SHAPES = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13)}


@gpu
@pytest.mark.parametrize("shape", [(n, c, *HW_SHAPES[hw]) for n, c in ((1, 1), (1, 5), (7, 1))
                                   for hw in (1, 63, 64, 65)] + [(2, 3, 17, 241)])
def test_avgpool_segate_remainders_saturated_gates(shape):
    """k_avgpool_fwd / k_se_gate_bwd (csrc/pool.hip:69-78, 97-114) with HW in {1, 63, 64, 65,
    4097} and plane counts that are no multiple of the 4 waves of a block; gate logits of +-20
    and +-100 among ordinary ones (sigmoid saturates, s (1 - s) underflows) and planes offset
    by up to +-100.  Bound: test_maxpool_avgpool_segate's 1e-6 under the `_bound` rule."""
    from e2ep_amd import nn_ops
    N, C, H, W = shape
    g = _g(sum(shape))
    off = (torch.rand(N, C, 1, 1, generator=g) * 2 - 1) * 100
    x = torch.randn(*shape, generator=g) + off
    a = torch.tensor([GATES[i % len(GATES)] for i in range(N * C)]).view(N, C, 1, 1)
    a = a + 0.01 * torch.randn(N, C, 1, 1, generator=g)
    dy = torch.randn(*shape, generator=g)
    xd, ad = x.to(DEV).requires_grad_(True), a.to(DEV).requires_grad_(True)
    out = nn_ops.se_gate(xd, ad) + nn_ops.global_avg_pool(xd)
    out.backward(dy.to(DEV))
    refs = []
    for dt in (torch.float64, torch.float32):
        xr, ar = x.to(dt).requires_grad_(True), a.to(dt).requires_grad_(True)
        o = xr * torch.sigmoid(ar) + xr.mean((2, 3), keepdim=True)
        o.backward(dy.to(dt))
        refs.append((o.detach(), xr.grad, ar.grad))
    for name, got, r64, r32 in zip(("out", "dx", "da"), (out, xd.grad, ad.grad), *refs):
        _check(f"avgpool+se_gate {shape} {name}", got, r64, r32, 1e-6)


# ------------------------------------------------------------------------------------------
# 4. channel softmax: C limit, saturation, -inf, NaN
# ------------------------------------------------------------------------------------------
SM_PIX = {1: (1, 1, 1), 65: (1, 5, 13), 130: (2, 5, 13)}


def _softmax_input(C, npix, kind):
    N, H, W = SM_PIX[npix]
    g = _g(C * 1000 + npix + len(kind))
    x = torch.randn(N, C, H, W, generator=g) * 3
    if kind == "big":
        x = x * 1e4
    elif kind == "neg_inf":
        if C > 1:  # channel 0 stays finite: no column is entirely -inf
            x[:, 1:][torch.rand(N, C - 1, H, W, generator=g) < 0.4] = -INF
    else:
        assert kind == "equal"
        x = x[:, :1].expand(N, C, H, W).contiguous()
    return x, torch.randn(N, C, H, W, generator=g)


@gpu
@pytest.mark.parametrize("kind", ["big", "neg_inf", "equal"])
@pytest.mark.parametrize("npix", [1, 65, 130])
@pytest.mark.parametrize("C", [1, 2, 63, 64])
def test_softmax_channels_saturated_inf_equal(C, npix, kind):
    """k_softmax_c_fwd / _bwd (csrc/pool.hip:185-233) up to the C == 64 register limit, one pixel
    and pixel counts that are no multiple of the 64-thread block: logits scaled by 1e4 (exact
    zeros and ones), columns with -inf entries, all-equal columns; vs fp64 softmax(1) at
    test_softmax_channels_vs_fp64's bounds (1e-6 forward, 1e-5 backward)."""
    from e2ep_amd import nn_ops
    x, dy = _softmax_input(C, npix, kind)
    xd = x.to(DEV).requires_grad_(True)
    y = nn_ops.softmax_channels(xd)
    (y * dy.to(DEV)).sum().backward()
    x64 = x.double().requires_grad_(True)
    y64 = x64.softmax(1)
    (y64 * dy.double()).sum().backward()
    x32 = x.clone().requires_grad_(True)
    y32 = x32.softmax(1)
    (y32 * dy).sum().backward()
    # one-hot columns: dx = y (dy - sum y dy) cancels to rounding noise in fp32, torch's too
    tag = f"softmax_c C={C} pixels={npix} {kind}"
    _check(f"{tag} y", y, y64, y32, 1e-6)
    _check(f"{tag} dx", xd.grad, x64.grad, x32.grad, 1e-5)
    # absolute form, which stays meaningful when the whole gradient is such noise: y <= 1 and the
    # C-term fp32 sum of y dy is off by at most C ulp of max |dy|
    worst = float((xd.grad.cpu().double() - x64.grad).abs().max())
    assert worst <= C * 2.0 ** -23 * float(dy.abs().max()), worst
    assert torch.isfinite(y).all() and torch.isfinite(xd.grad).all()
    yc, y64 = y.detach().cpu(), y64.detach()
    if kind == "big":  # exactly 1 / exactly 0 where the fp64 reference is
        assert bool((yc[y64 == 1] == 1).all()) and bool((yc[y64 == 0] == 0).all())
        if npix > 1:
            assert bool((y64 == 1).any()) and (C == 1 or bool((y64 == 0).any()))
    if kind == "neg_inf":
        assert bool((yc[torch.isinf(x)] == 0).all())
        assert bool((xd.grad.cpu()[torch.isinf(x)] == 0).all())
    if kind == "equal":
        assert torch.equal(yc, torch.full_like(yc, 1.0 / C))


@gpu
@pytest.mark.parametrize("C", [2, 64])
def test_softmax_channels_nan_where_torch_is_nan(C):
    """A column that is entirely -inf and a column holding +inf: NaN wherever torch's fp32 CPU
    softmax is NaN; the other columns are unaffected."""
    from e2ep_amd import nn_ops
    x = torch.randn(2, C, 5, 13, generator=_g(C)) * 3
    x[0, :, 0, 3] = -INF
    x[1, C // 2, 2, 7] = INF
    y = nn_ops.softmax_channels(x.to(DEV)).cpu()
    ref = x.softmax(1)
    nan = torch.isnan(ref)
    assert int(nan.sum()) == 2 * C
    assert bool(torch.isnan(y[nan]).all())
    assert not bool(torch.isnan(y[~nan]).any())
    assert rel_l2(y[~nan], x.double().softmax(1)[~nan]) < 1e-6


@gpu
def test_softmax_channels_refuses_65_channels():
    """C = 65 is past the kernel's register column (SMC_MAX, csrc/pool.hip:184, 240): E2EPError,
    and the output buffer is not written."""
    from e2ep_amd import _lib, nn_ops
    x = torch.randn(1, 65, 5, 13, device=DEV)
    y = torch.full_like(x, 7.0)
    with pytest.raises(_lib.E2EPError):
        _lib.call("e2ep_softmax_c_fwd", _lib.ptr(x), 1, 65, 65, _lib.ptr(y), _lib.stream())
    with pytest.raises(_lib.E2EPError):
        _lib.call("e2ep_softmax_c_bwd", _lib.ptr(x), _lib.ptr(x), 1, 65, 65, _lib.ptr(y), _lib.stream())
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    with pytest.raises(_lib.E2EPError):
        nn_ops.softmax_channels(x)


# ------------------------------------------------------------------------------------------
# 5. losses: upstream gradient, saturation, -inf, degenerate counts
# ------------------------------------------------------------------------------------------
GL = 0.37  # the upstream gradient of loss.backward(): every other loss test passes 1


def _oracle():
    from oracle import parking_ref as O
    return O


def _value_close(out, ref):
    out, ref = float(out), float(ref)
    if ref == 0.0:
        return out == 0.0
    return abs(out / ref - 1) < 1e-6


def _control_case(V, kind):
    B, T, pad = 3, 14, V - 1
    g = _g(V + len(kind))
    pred = torch.randn(B, T, V, generator=g) * 3
    gt = torch.randint(0, V - 1, (B, T + 1), generator=g)
    gt[0, 9:] = pad
    if kind == "big":
        pred = pred * 1e4
    elif kind == "neg_inf":
        hole = torch.rand(B, T, V, generator=g) < 0.3
        hole.scatter_(2, gt[:, 1:].unsqueeze(-1), False)  # never the target entry
        pred[hole] = -INF
    else:
        assert kind == "one_row"
        gt[:, 1:] = pad
        gt[1, 5] = V // 2
    return pred, gt, pad


@gpu
@pytest.mark.parametrize("kind", ["big", "neg_inf", "one_row"])
@pytest.mark.parametrize("V", [7, 64, 65, 204])
def test_control_ce_value_edges(V, kind):
    """k_ctrl_ce_rows / _bwd (csrc/loss.hip:35-96) at vocabularies around the 64-lane row stride,
    with logits scaled by 1e4, -inf at non-target entries, and a batch whose only non-PAD row is
    one; backward through 0.37 * loss (the gloss argument).  Oracle in fp64, bounds of
    test_losses_gpu.py (1e-6 on the value, rel-L2 1e-6 on the gradient)."""
    from e2ep_amd import losses
    O = _oracle()
    pred, gt, pad = _control_case(V, kind)
    ref_in = pred.double().requires_grad_()
    ref = O.control_loss(ref_in, gt, pad)
    (GL * ref).backward()
    x = pred.to(DEV).requires_grad_()
    out = losses.control_ce(x, gt.to(DEV), pad)
    (GL * out).backward()
    e = rel_l2(x.grad, ref_in.grad)
    print(f"control_ce V={V} {kind}: loss {float(out):.8g} vs {float(ref):.8g}, grad rel-L2 {e:.3e}")
    assert _value_close(out, ref)
    assert torch.isfinite(x.grad).all()
    assert e < 1e-6
    if kind == "one_row":
        rows = x.grad.abs().sum(-1).cpu() != 0
        assert int(rows.sum()) == 1 and bool(rows[1, 4])


@gpu
@pytest.mark.parametrize("kind", ["plain", "all_ignored", "zero_weight"])
@pytest.mark.parametrize("hw", [(1, 1), (15, 17), (1, 257)])
def test_seg_ce_value_edges(hw, kind):
    """k_seg_ce_fwd / _bwd (csrc/loss.hip:100-164) at pixel counts 1, 255, 257 (the 256-thread
    block boundary): every pixel ignored (loss and gradient exactly 0), a class weight of 0,
    backward through 0.37 * loss."""
    from e2ep_amd import losses
    O = _oracle()
    h, w = hw
    g = _g(h * w + len(kind))
    pred = torch.randn(1, 1, 3, h, w, generator=g) * 2
    tgt = torch.randint(0, 3, (1, 1, h, w), generator=g)
    weights = (1.0, 0.0, 2.0) if kind == "zero_weight" else (1.0, 2.0, 2.0)
    if kind == "all_ignored":
        tgt[:] = 255
    elif h * w > 1:
        tgt[0, 0, 0, 0] = 255
    ref_in = pred.double().requires_grad_()
    ref = O.segmentation_loss(ref_in, tgt, weights)
    (GL * ref).backward()
    x = pred.to(DEV).requires_grad_()
    out = losses.seg_weighted_ce(x, tgt.to(DEV), torch.tensor(weights))
    (GL * out).backward()
    assert _value_close(out, ref)
    assert rel_l2(x.grad, ref_in.grad) < 1e-6
    assert torch.isfinite(out).all() and torch.isfinite(x.grad).all()
    if kind == "all_ignored":
        assert float(out) == 0.0 and float(ref) == 0.0
        assert float(x.grad.abs().max()) == 0.0
    if kind == "zero_weight":
        zero = (tgt[0] == 1).expand(3, h, w)  # pixels of the weight-0 class: no gradient
        assert float((x.grad[0, 0].cpu() * zero).abs().max()) == 0.0


DEPTH_BOUND, DOWN = (0.5, 12.5, 0.25), 8


@gpu
def test_depth_bce_no_foreground():
    """max(1, #foreground) with no foreground cell (k_loss_final, csrc/loss.hip:136): loss exactly
    0, den == 1, gradient exactly 0."""
    from e2ep_amd import losses
    O = _oracle()
    prob = torch.randn(2, 48, 32, 32, generator=_g(3)).softmax(1)
    depth = torch.zeros(1, 2, 256, 256)
    ref = O.depth_loss(prob.double(), depth.double())
    x = prob.to(DEV).requires_grad_()
    out = losses.depth_bce(x, depth.to(DEV), DEPTH_BOUND, DOWN)
    den = out.grad_fn.saved_tensors[2]
    (GL * out).backward()
    assert float(out) == 0.0 and float(ref) == 0.0
    assert float(den) == 1.0
    assert float(x.grad.abs().max()) == 0.0 and torch.isfinite(x.grad).all()


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["depth_fp32", "depth_fp64"])
def test_depth_bce_saturated_probabilities(dtype):
    """bce_term's log clamp at -100 and the backward's 1e-12 clamp (csrc/loss.hip:169-172,
    229-232): probabilities of exactly 0 and exactly 1, on the labelled bin and off it, in
    foreground cells; the fp64 oracle gives 100 per saturated term and +-scale / 1e-12
    gradients.  The gradient is also compared without the planted entries, which otherwise
    dominate the norm."""
    from e2ep_amd import losses
    O = _oracle()
    g = _g(11)
    prob = torch.randn(2, 48, 32, 32, generator=g).softmax(1)
    # one depth level per 8 x 8 cell (plus 0.2 m of spread), so most cells are foreground
    depth = torch.rand(1, 2, 32, 32, generator=g, dtype=dtype) * 14.0
    depth = depth.repeat_interleave(8, 2).repeat_interleave(8, 3)
    depth = depth + 0.2 * torch.rand(1, 2, 256, 256, generator=g, dtype=dtype)
    depth[0, 0, :64, :64] = 0.0
    lab = O.depth_labels(depth.double()).view(2, 32, 32, 48)
    cells = (lab.max(-1).values > 0).nonzero()[::97][:8]
    assert len(cells) == 8
    planted = torch.zeros_like(prob, dtype=torch.bool)
    for i, (bn, ci, cj) in enumerate(cells.tolist()):
        k = int(lab[bn, ci, cj].argmax())
        d = k if i % 2 == 0 else (k + 5) % 48      # on the labelled bin / off it
        prob[bn, d, ci, cj] = float((i // 2) % 2)  # exactly 0 / exactly 1
        planted[bn, d, ci, cj] = True
    ref_in = prob.double().requires_grad_()
    ref = O.depth_loss(ref_in, depth.double())
    (GL * ref).backward()
    x = prob.to(DEV).requires_grad_()
    out = losses.depth_bce(x, depth.to(DEV), DEPTH_BOUND, DOWN)
    (GL * out).backward()
    gk, gr = x.grad.cpu(), ref_in.grad
    assert float(gr[planted].abs().max()) > 1e6  # the 1e-12 clamp was reached
    assert _value_close(out, ref)
    assert torch.isfinite(gk).all()
    assert rel_l2(gk, gr) < 1e-6
    assert rel_l2(gk[~planted], gr[~planted]) < 1e-6


@gpu
def test_three_losses_summed_as_the_train_step():
    """The train step's sum3(control, segmentation, depth) (trainer/pl_trainer.py), scaled by
    0.37: every loss's backward receives its upstream gradient from the sum's backward."""
    from e2ep_amd import losses, nn_ops
    O = _oracle()
    g = _g(21)
    pc, gt, pad = _control_case(204, "one_row")
    gt[2, 1:6] = torch.randint(0, 200, (5,), generator=g)
    ps = torch.randn(1, 1, 3, 15, 17, generator=g) * 2
    tg = torch.randint(0, 3, (1, 1, 15, 17), generator=g)
    pd = torch.randn(2, 48, 32, 32, generator=g).softmax(1)
    depth = torch.rand(1, 2, 256, 256, generator=g) * 15.0
    r = [t.double().requires_grad_() for t in (pc, ps, pd)]
    ref = O.control_loss(r[0], gt, pad) + O.segmentation_loss(r[1], tg) + O.depth_loss(r[2], depth.double())
    (GL * ref).backward()
    d = [t.to(DEV).requires_grad_() for t in (pc, ps, pd)]
    out = nn_ops.sum3(losses.control_ce(d[0], gt.to(DEV), pad),
                      losses.seg_weighted_ce(d[1], tg.to(DEV), torch.tensor([1.0, 2.0, 2.0])),
                      losses.depth_bce(d[2], depth.to(DEV), DEPTH_BOUND, DOWN))
    (GL * out).backward()
    assert _value_close(out, ref)
    for a, b in zip(d, r):
        assert rel_l2(a.grad, b.grad) < 1e-6


# ------------------------------------------------------------------------------------------
# 6. BatchNorm under offset channel means, every path
# ------------------------------------------------------------------------------------------
BN_SHAPES = [(8, 24, 16, 16), (3, 7, 5, 9), (4, 24, 32, 32)]
BN_BASE = dict(out=1e-6, dx=1e-5, dgamma=1e-5, dbeta=1e-5, rm=1e-6, rv=1e-6)  # test_bn_act's


def _channel_means(C, g):
    """Per-channel means spread over [-100, 100], both ends included, in a shuffled order."""
    mu = torch.linspace(-100, 100, C) if C > 1 else torch.tensor([100.0])
    return mu[torch.randperm(C, generator=g)]


def _offset_input(shape):
    """x = randn + mu_c (sigma 1), BN weight / bias and an output gradient; CPU fp32."""
    g = _g(sum(shape))
    C = shape[1]
    x = torch.randn(*shape, generator=g) + _channel_means(C, g).view(1, C, 1, 1)
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    return x, gamma, beta, torch.randn(*shape, generator=g)


def _bn_ref(x, gamma, beta, dy, dtype, post=None, extra=()):
    """Training F.batch_norm (running statistics from 0 / 1) then `post`, on the CPU in `dtype`."""
    C = x.shape[1]
    xr, gr, br = (t.detach().cpu().to(dtype).requires_grad_(True) for t in (x, gamma, beta))
    ex = [t.detach().cpu().to(dtype) for t in extra]
    rm, rv = torch.zeros(C, dtype=dtype), torch.ones(C, dtype=dtype)
    z = F.batch_norm(xr, rm, rv, gr, br, True, MOM, EPS)
    y = post(z, *ex) if post else z
    y.backward(dy.detach().cpu().to(dtype))
    return dict(out=y.detach(), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad, rm=rm, rv=rv)


def _bn_module(gamma, beta):
    bn = nn.BatchNorm2d(gamma.numel(), momentum=MOM, eps=EPS)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    return bn.to(DEV).train()


def _bn_compare(tag, got, x, gamma, beta, dy, post=None, extra=()):
    r64 = _bn_ref(x, gamma, beta, dy, torch.float64, post, extra)
    r32 = _bn_ref(x, gamma, beta, dy, torch.float32, post, extra)
    for k, base in BN_BASE.items():
        _check(f"{tag} {k}", got[k], r64[k], r32[k], base)


def _bn_got(out, xd, bn):
    return dict(out=out, dx=xd.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, rm=bn.running_mean,
                rv=bn.running_var)


def _one_pass_fp32(x, gamma, beta):
    """The failure the offset inputs target: fp32 sums and var = E[x^2] - m^2."""
    m = x.mean((0, 2, 3), keepdim=True)
    var = ((x * x).mean((0, 2, 3), keepdim=True) - m * m).clamp_min(0)
    return (x - m) / torch.sqrt(var + EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)


@pytest.mark.parametrize("shape", BN_SHAPES)
def test_offset_inputs_separate_one_pass_variance_from_fp32(shape):
    """CPU only.  On the inputs of the BatchNorm tests below, torch's fp32 F.batch_norm stays
    within the bound those tests apply to the output, and an fp32 one-pass E[x^2] - m^2
    emulation breaks it by at least 10 x: the inputs tell the failure from the reference."""
    x, gamma, beta, _ = _offset_input(shape)
    y64 = F.batch_norm(x.double(), None, None, gamma.double(), beta.double(), True, 0.0, EPS)
    e32 = rel_l2(F.batch_norm(x, None, None, gamma, beta, True, 0.0, EPS), y64)
    e1p = rel_l2(_one_pass_fp32(x, gamma, beta), y64)
    bound = _bound(BN_BASE["out"], e32)
    print(f"{shape}: torch fp32 {e32:.3e}, bound {bound:.3e}, fp32 one-pass {e1p:.3e}")
    assert e32 <= bound
    assert e1p >= 10 * bound


@gpu
@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_act_offset_means(shape, bn_path):  # noqa: F811
    """batch_norm_act in train mode on both BN paths (csrc/bn.hip: the single-launch
    block-per-channel kernels and the split statistics + apply kernels), fp64 statistics and
    var = Q / cnt - m^2: output, input / weight / bias gradients and running statistics."""
    from e2ep_amd import nn_ops
    x, gamma, beta, dy = _offset_input(shape)
    bn = _bn_module(gamma, beta)
    xd = x.to(DEV).requires_grad_(True)
    y = nn_ops.batch_norm_act(xd, bn, None)
    y.backward(dy.to(DEV))
    _bn_compare(f"bn_act {shape} small={bn_path}", _bn_got(y, xd, bn), x, gamma, beta, dy)


def _se_post(z, w1, b1, w2, b2):
    u = z * torch.sigmoid(z)
    h = F.conv2d(F.adaptive_avg_pool2d(u, 1), w1, b1)
    return u * torch.sigmoid(F.conv2d(h * torch.sigmoid(h), w2, b2))


def _se_params(C, sq, g):
    return (torch.randn(sq, C, 1, 1, generator=g) / C ** 0.5, torch.randn(sq, generator=g) * 0.1,
            torch.randn(C, sq, 1, 1, generator=g) / sq ** 0.5, torch.randn(C, generator=g) * 0.1)


@gpu
@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_swish_se_offset_means(shape, bn_path, se_bn_sums):  # noqa: F811
    """bn_swish_squeeze_excite (BN + swish applied on load by the SE kernels; backward sums from
    the SE pass or the BN's own reduction) under offset channel means."""
    from e2ep_amd import nn_ops
    x, gamma, beta, dy = _offset_input(shape)
    se = _se_params(shape[1], 4, _g(5))
    bn = _bn_module(gamma, beta)
    xd = x.to(DEV).requires_grad_(True)
    y = nn_ops.bn_swish_squeeze_excite(xd, bn, *[t.to(DEV) for t in se])
    y.backward(dy.to(DEV))
    _bn_compare(f"bn_swish_se {shape} small={bn_path} se_sums={se_bn_sums}", _bn_got(y, xd, bn), x,
                gamma, beta, dy, _se_post, se)


@gpu
def test_bn_from_conv_partials_offset_means():
    """BatchNorm fed the 1x1 conv epilogue's fp64 partial sums (test_bn_stats_gpu.py's
    construction; bnstats.h).  The conv output carries the offsets: one input channel is
    constant 1 and its weights are the channel means.  Reference: fp64 BatchNorm of the conv's
    own fp32 output."""
    from e2ep_amd import conv, nn_ops
    g = _g(7)
    N, Cin, H, W, Cout = 16, 32, 32, 32, 192
    x0 = torch.randn(N, Cin, H, W, generator=g)
    x0[:, -1] = 1.0
    w0 = torch.randn(Cout, Cin, 1, 1, generator=g) / (Cin - 1) ** 0.5
    w0[:, -1, 0, 0] = _channel_means(Cout, g)
    gamma = 1 + 0.3 * torch.randn(Cout, generator=g)
    beta = 0.2 * torch.randn(Cout, generator=g)
    dy = torch.randn(N, Cout, H, W, generator=g)
    bn = _bn_module(gamma, beta)
    y = conv.conv2d(x0.to(DEV).requires_grad_(True), w0.to(DEV), bn_stats=True)
    assert conv.bn_partials(y) is not None
    y.retain_grad()
    out = nn_ops.batch_norm_act(y, bn, None)
    out.backward(dy.to(DEV))
    m = y.detach().mean((0, 2, 3)).cpu()
    assert float(m.min()) < -99 and float(m.max()) > 99
    _bn_compare("bn from conv partials", _bn_got(out, y, bn), y, gamma, beta, dy)


@gpu
def test_bn_swish_se_from_depthwise_partials_offset_means():
    """_bn1 + swish + SE fed the depthwise kernel's fp64 partial sums; the depthwise weights are
    the centre tap alone, so its output is the offset input.  Reference: fp64 on the depthwise
    conv's own fp32 output."""
    from e2ep_amd import conv, nn_ops
    g = _g(11)
    N, C, H, W, sq = 12, 144, 32, 32, 6
    x0 = torch.randn(N, C, H, W, generator=g) + _channel_means(C, g).view(1, C, 1, 1)
    wd = torch.zeros(C, 1, 3, 3)
    wd[:, 0, 1, 1] = 1.0
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    se = _se_params(C, sq, g)
    dy = torch.randn(N, C, H, W, generator=g)
    bn = _bn_module(gamma, beta)
    y = nn_ops.depthwise_conv2d(x0.to(DEV).requires_grad_(True), wd.to(DEV), 1, (1, 1, 1, 1), bn_stats=True)
    assert conv.bn_partials(y) is not None
    assert torch.equal(y.detach().cpu(), x0)
    y.retain_grad()
    out = nn_ops.bn_swish_squeeze_excite(y, bn, *[t.to(DEV) for t in se])
    out.backward(dy.to(DEV))
    _bn_compare("bn_swish_se from depthwise partials", _bn_got(out, y, bn), y, gamma, beta, dy, _se_post, se)


def _swish(z):
    return z * torch.sigmoid(z)


def _mid_ref(x, gy, p, K, dtype):
    """The MBConv middle (test_mbconv_mid_gpu._ref64's chain) with running statistics, in `dtype`."""
    C = x.shape[1]
    q = {k: v.to(dtype).requires_grad_(True) for k, v in p.items()}
    xr = x.to(dtype).requires_grad_(True)
    rm0, rv0, rm1, rv1 = (f(C, dtype=dtype) for f in (torch.zeros, torch.ones, torch.zeros, torch.ones))
    a0 = _swish(F.batch_norm(xr, rm0, rv0, q["g0"], q["b0"], True, MOM, EPS))
    y1 = F.conv2d(a0, q["w"], padding=K // 2, groups=C)
    a1 = _swish(F.batch_norm(y1, rm1, rv1, q["g1"], q["b1"], True, MOM, EPS))
    a = F.conv2d(_swish(F.conv2d(a1.mean((2, 3), keepdim=True), q["w1"], q["sb1"])), q["w2"], q["sb2"])
    y = a1 * torch.sigmoid(a)
    y.backward(gy.to(dtype))
    return dict(y=y.detach(), dx=xr.grad, dg0=q["g0"].grad, db0=q["b0"].grad, dg1=q["g1"].grad,
                db1=q["b1"].grad, rm0=rm0, rv0=rv0, rm1=rm1, rv1=rv1)


@gpu
def test_mbconv_mid_offset_means():
    """The fused MBConv middle (csrc/mbconv_mid.hip) at its smallest accepted 16x16 case
    (N 1, C 3, k 3) with channel means -100 / 0 / 100: output, input gradient, both BatchNorms'
    weight / bias gradients and running statistics vs fp64."""
    import test_mbconv_mid_gpu as M
    from e2ep_amd import ops
    N, C, K = 1, 3, 3
    g = _g(36)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = r(N, C, 16, 16) + torch.tensor([-100.0, 0.0, 100.0]).view(1, C, 1, 1)
    gy = r(N, C, 16, 16)
    p = dict(g0=1 + 0.1 * r(C), b0=0.1 * r(C), g1=1 + 0.1 * r(C), b1=0.1 * r(C), w=r(C, 1, K, K) / K,
             w1=r(2, C, 1, 1) / C ** 0.5, sb1=0.1 * r(2), w2=r(C, 2, 1, 1), sb2=0.1 * r(C))
    prev = M._tune(M.KEY, 2)
    try:
        layers = M._layers(C, K, p)
        bn0, dw, bn1 = layers[:3]
        xd = x.to(DEV).requires_grad_(True)
        assert ops.mbconv_mid_ok(xd.shape, xd.dtype, bn0, dw, bn1)
        y = M._forward(xd, layers)[0]
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
    finally:
        M._tune(M.KEY, prev)
    got = dict(y=y, dx=xd.grad, dg0=bn0.weight.grad, db0=bn0.bias.grad, dg1=bn1.weight.grad,
               db1=bn1.bias.grad, rm0=bn0.running_mean, rv0=bn0.running_var, rm1=bn1.running_mean,
               rv1=bn1.running_var)
    r64, r32 = _mid_ref(x, gy, p, K, torch.float64), _mid_ref(x, gy, p, K, torch.float32)
    base = dict(y=1e-6, dx=1e-5, dg0=1e-5, db0=1e-5, dg1=1e-5, db1=1e-5, rm0=1e-6, rv0=1e-6, rm1=1e-6,
                rv1=1e-6)  # test_bn_swish_depthwise_fused / test_bn_swish_se_fused
    for k, b in base.items():
        _check(f"mbconv_mid {k}", got[k], r64[k], r32[k], b)


# ------------------------------------------------------------------------------------------
# 7. LayerNorm: the E limit, constant rows, offset rows
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["plain", "constant", "offset"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("E", [1, 64, 65, 512])
def test_add_layernorm_limits_constant_offset(E, rows, kind):
    """add_dropout_layernorm with p = 0 (csrc/ln.hip) at E = 1, the 64-lane row stride +- 1 and
    the E == 512 limit; row counts below and above the 4 rows of a block; rows whose a + b is
    constant (variance exactly 0) and rows with a mean of 1e3 and unit spread.  vs fp64
    layer_norm(a + b) at test_add_dropout_layernorm_fused's bounds (1e-6, gradients 1e-5)."""
    from e2ep_amd import nn_ops
    g = _g(E * 10 + rows + len(kind))
    a = torch.randn(rows, E, generator=g)
    b = torch.randn(rows, E, generator=g)
    if kind == "constant":
        a = torch.randint(-8, 9, (rows, E), generator=g).float()
        b = 3.0 - a                                  # a + b == 3 exactly in fp32
    elif kind == "offset":
        a = a + 1e3
    gamma = 1 + 0.2 * torch.randn(E, generator=g)
    beta = 0.1 * torch.randn(E, generator=g)
    dy = torch.randn(rows, E, generator=g)
    ts = [t.to(DEV).requires_grad_(True) for t in (a, b, gamma, beta)]
    y = nn_ops._AddDropLN.apply(ts[0], ts[1], ts[2], ts[3], None, None, 0.0, 1e-5)
    y.backward(dy.to(DEV))
    refs = []
    for dt in (torch.float64, torch.float32):
        rs = [t.to(dt).requires_grad_(True) for t in (a, b, gamma, beta)]
        yr = F.layer_norm(rs[0] + rs[1], (E,), rs[2], rs[3], 1e-5)
        yr.backward(dy.to(dt))
        refs.append([yr.detach()] + [t.grad for t in rs])
    got = [y] + [t.grad for t in ts]
    assert all(bool(torch.isfinite(t).all()) for t in got)
    for name, base, k, r64, r32 in zip(("y", "da", "db", "dgamma", "dbeta"), (1e-6,) + (1e-5,) * 4, got,
                                       *refs):
        if E == 1 and name != "dbeta":
            # a one-element row is its own mean: y = beta and da = db = dgamma = 0 exactly (torch's
            # own results carry rounding noise around 0 here, so they are no reference)
            want = beta.expand(rows, E) if name == "y" else torch.zeros_like(r64, dtype=torch.float32)
            assert torch.equal(k.detach().cpu(), want), name
            continue
        _check(f"layernorm E={E} rows={rows} {kind} {name}", k, r64, r32, base)


@gpu
def test_add_layernorm_refuses_513():
    """E = 513 is past the kernel's 64 x LN_MAXV row (csrc/ln.hip:168, 201): E2EPError."""
    from e2ep_amd import _lib, nn_ops
    ts = [torch.randn(2, 513, device=DEV), torch.randn(2, 513, device=DEV), torch.ones(513, device=DEV),
          torch.zeros(513, device=DEV)]
    with pytest.raises(_lib.E2EPError):
        nn_ops._AddDropLN.apply(ts[0], ts[1], ts[2], ts[3], None, None, 0.0, 1e-5)


# ------------------------------------------------------------------------------------------
# 8. attention with saturated scores
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Sq,Sk,causal,base", [(14, 14, True, 1e-4), (14, 256, False, 1e-4),
                                               (128, 128, False, 1e-5)],
                         ids=["self_causal_14", "cross_14x256", "matrix_core_128"])
def test_attention_saturated_scores(Sq, Sk, causal, base):
    """q scaled by 30: the softmax rows are near one-hot (scores of std ~30), p = 0.  The vector
    kernels (csrc/attn.hip; causal 14 x 14 and cross 14 x 256) at
    test_attention_dropout_matches_masked_reference's 1e-4 and the matrix-core kernels
    (csrc/attn_mf.hip, 128 x 128, e2ep_tune key 21 = 3) at
    test_attention_matrix_core_matches_reference's 1e-5, against that file's fp64 restatement;
    `_bound` applies with the same restatement in fp32."""
    from test_attention_gpu import H, _ref_core
    from e2ep_amd import _lib, attention
    g = _g(Sq + Sk)
    B, dh = 4, 43
    Ed = H * dh
    qb = torch.randn(Sq, B, Ed, generator=g) * 30
    kvb = torch.randn(Sk, B, 2 * Ed, generator=g)
    do = torch.randn(Sq, B, Ed, generator=g)
    old = _lib.call_raw("e2ep_tune", 21, 3)
    try:
        qd = qb.to(DEV).requires_grad_(True)
        kvd = kvb.to(DEV).requires_grad_(True)
        o = attention.attention(qd, kvd, H, causal, None, 0.0, None)
        (o * do.to(DEV)).sum().backward()
    finally:
        _lib.call_raw("e2ep_tune", 21, old)

    def heads(t):  # (S, B, H*dh) -> (B*H, S, dh)
        S = t.shape[0]
        return t.reshape(S, B, H, dh).permute(1, 2, 0, 3).reshape(B * H, S, dh)
    refs = []
    for dt in (torch.float64, torch.float32):
        qr = qb.to(dt).requires_grad_(True)
        kvr = kvb.to(dt).requires_grad_(True)
        keep = torch.ones(B * H, Sq, Sk, dtype=dt)
        orr = _ref_core(heads(qr), heads(kvr[..., :Ed]), heads(kvr[..., Ed:]), keep, 0.0, causal, None)
        orr = orr.reshape(B, H, Sq, dh).permute(2, 0, 1, 3).reshape(Sq, B, Ed)
        (orr * do.to(dt)).sum().backward()
        refs.append((orr.detach(), qr.grad, kvr.grad[..., :Ed], kvr.grad[..., Ed:]))
    P = torch.softmax(heads(qb.double()) @ heads(kvb[..., :Ed].double()).transpose(1, 2) / math.sqrt(dh), -1)
    if not causal:
        assert float(P.max(-1).values.median()) > 0.9  # near one-hot
    got = (o, qd.grad, kvd.grad[..., :Ed], kvd.grad[..., Ed:])
    for name, k, r64, r32 in zip(("o", "dq", "dk", "dv"), got, *refs):
        _check(f"attention {Sq}x{Sk} {name}", k, r64, r32, base)
