"""The MBConv middle on 16x16 maps as one launch per direction (csrc/mbconv_mid.hip,
e2ep_tune key 36): _bn0 -> swish -> depthwise -> _bn1 -> swish -> SE squeeze, and its backward.

Every case runs the chain with the key on (fused) and off (the separate launches) on the same
inputs.  The fused kernels repeat the separate kernels' arithmetic and summation order, so
every output must be bitwise equal, except the depthwise weight gradient where the separate
kernel sums several split slabs per channel (channel counts under 512): the fused kernel repeats
the one-split order (bitwise equal there, as in the 16x16 stages).  That gradient's error
against a float64 torch restatement must stay within twice the separate path's own error on the
same inputs (both are fp32 roundings of the same sums; 2x leaves room for the reordered sum).
Both errors are printed."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEY = 36
EPS, MOM = 1e-3, 0.01  # efficientnet-pytorch's BatchNorm settings

# (N, C, K): one plane per channel (most waves idle); k5; a plane count that is no multiple of
# the wave count; the 8192-element limit
CASES = [(1, 3, 3), (2, 5, 5), (5, 8, 3), (32, 8, 5)]
IDS = ["n1c3k3", "n2c5k5", "n5c8k3", "n32c8k5"]
BITWISE = ["y", "y1", "st0", "st1", "pooled", "rm0", "rv0", "rm1", "rv1", "dx", "dg0", "db0", "dg1",
           "db1", "dw1", "dsb1", "dw2", "dsb2"]


def _tune(key, value):
    from e2ep_amd import _lib
    return _lib.load().e2ep_tune(key, value)


@functools.lru_cache(maxsize=None)
def _inputs(N, C, K):
    """Input, output gradient and parameters (CPU, fp32).  Channel 0 is constant (variance 0);
    channel 1 has mean 100 and std 0.1, where fp32 sums would lose the variance."""
    g = torch.Generator().manual_seed(1000 * N + 10 * C + K)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = r(N, C, 16, 16)
    x[:, 0] = 0.7
    x[:, 1] = 100.0 + 0.1 * r(N, 16, 16)
    sq = 2
    p = dict(g0=1 + 0.1 * r(C), b0=0.1 * r(C), g1=1 + 0.1 * r(C), b1=0.1 * r(C), w=r(C, 1, K, K) / K,
             w1=r(sq, C, 1, 1) / C ** 0.5, sb1=0.1 * r(sq), w2=r(C, sq, 1, 1), sb2=0.1 * r(C))
    return x, r(N, C, 16, 16), p


def _layers(C, K, p):
    from model.efficientnet import SameConv
    from torch import nn
    bn0 = nn.BatchNorm2d(C, momentum=MOM, eps=EPS)
    bn1 = nn.BatchNorm2d(C, momentum=MOM, eps=EPS)
    dw = SameConv(C, C, K, 1, groups=C, bias=False, size=16)
    red, exp = SameConv(C, p["w1"].shape[0], 1), SameConv(p["w1"].shape[0], C, 1)
    with torch.no_grad():
        for t, k in ((bn0.weight, "g0"), (bn0.bias, "b0"), (bn1.weight, "g1"), (bn1.bias, "b1"),
                     (dw.weight, "w"), (red.weight, "w1"), (red.bias, "sb1"), (exp.weight, "w2"),
                     (exp.bias, "sb2")):
            t.copy_(p[k])
    return [m.to(DEV).train() for m in (bn0, dw, bn1, red, exp)]


def _forward(x, layers):
    """MBConv.forward's middle; (y, y1, st0, st1, pooled) with the statistics and the pooled
    means read from what the ops saved for their backward."""
    from e2ep_amd import ops
    bn0, dw, bn1, red, exp = layers
    if ops.mbconv_mid_ok(x.shape, x.dtype, bn0, dw, bn1):
        y = ops.mbconv_mid(x, bn0, dw, bn1, red, exp)
        s = y.grad_fn.saved_tensors
        return y, s[1], s[5], s[8], s[11]
    y1 = ops.bn_act_depthwise(x, bn0, "swish", dw, True)
    y = ops.bn_swish_squeeze_excite(y1, bn1, red, exp)
    s = y.grad_fn.saved_tensors
    return y, y1, y1.grad_fn.saved_tensors[4], s[3], s[6]


def _run(N, C, K, key, calls=1):
    """The chain forward + backward `calls` times on fresh layers with tune key 36 = key."""
    xc, gyc, p = _inputs(N, C, K)
    prev = _tune(KEY, key)
    try:
        layers = _layers(C, K, p)
        bn0, dw, bn1, red, exp = layers
        gy = gyc.to(DEV)
        for _ in range(calls):
            for m in layers:
                m.zero_grad(set_to_none=True)
            x = xc.to(DEV).requires_grad_(True)
            y, y1, st0, st1, pooled = _forward(x, layers)
            y.backward(gy)
        torch.cuda.synchronize()
    finally:
        _tune(KEY, prev)
    out = dict(y=y, y1=y1, st0=st0, st1=st1, pooled=pooled, rm0=bn0.running_mean,
               rv0=bn0.running_var, rm1=bn1.running_mean, rv1=bn1.running_var, dx=x.grad,
               dg0=bn0.weight.grad, db0=bn0.bias.grad, dg1=bn1.weight.grad, db1=bn1.bias.grad,
               dw=dw.weight.grad, dw1=red.weight.grad, dsb1=red.bias.grad, dw2=exp.weight.grad,
               dsb2=exp.bias.grad)
    return {k: v.detach().clone() for k, v in out.items()}


def _swish(z):
    return z * torch.sigmoid(z)


@functools.lru_cache(maxsize=None)
def _ref64(N, C, K):
    """float64 restatement of the chain (torch, CPU), computed once per case."""
    xc, gyc, p = _inputs(N, C, K)
    q = {k: v.double().requires_grad_(True) for k, v in p.items()}
    x = xc.double().requires_grad_(True)
    a0 = _swish(F.batch_norm(x, None, None, q["g0"], q["b0"], True, 0.0, EPS))
    y1 = F.conv2d(a0, q["w"], padding=K // 2, groups=C)
    a1 = _swish(F.batch_norm(y1, None, None, q["g1"], q["b1"], True, 0.0, EPS))
    pooled = a1.mean((2, 3), keepdim=True)
    a = F.conv2d(_swish(F.conv2d(pooled, q["w1"], q["sb1"])), q["w2"], q["sb2"])
    y = a1 * torch.sigmoid(a)
    y.backward(gyc.double())
    out = dict(y=y, y1=y1, pooled=pooled.flatten(1), dx=x.grad, dg0=q["g0"].grad, db0=q["b0"].grad,
               dg1=q["g1"].grad, db1=q["b1"].grad, dw=q["w"].grad, dw1=q["w1"].grad,
               dsb1=q["sb1"].grad, dw2=q["w2"].grad, dsb2=q["sb2"].grad)
    return {k: v.detach() for k, v in out.items()}


def _err(t, ref):
    """max |t - ref| / max |ref|"""
    return float((t.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _check_pair(on, off, ref, tag):
    for k in BITWISE:
        assert torch.equal(on[k], off[k]), f"{tag}: {k} differs from the separate launches"
    for k in sorted(ref):
        print(f"{tag} {k}: fused err {_err(on[k], ref[k]):.3e}, separate err {_err(off[k], ref[k]):.3e}")
    e_on, e_off = _err(on["dw"], ref["dw"]), _err(off["dw"], ref["dw"])
    assert e_on <= 2.0 * e_off, f"{tag}: depthwise weight gradient err {e_on:.3e} > 2 x {e_off:.3e}"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_equals_separate(case):
    from e2ep_amd import _lib
    N, C, K = case
    d = _lib.dims((N, C, 16, 16, K, 16, 16, 1, K // 2, K // 2))
    assert _lib.load().e2ep_mbconv_mid_ok(d) == 1
    on, off = _run(*case, 2), _run(*case, 1)
    _check_pair(on, off, _ref64(*case), f"N{N} C{C} k{K}")
    # the constant channel: variance 0, invstd = 1 / sqrt(eps)
    assert float(on["st0"][1, 0]) == pytest.approx(EPS ** -0.5, rel=1e-6)
    # the mean-100 channel: the fp64 statistics keep its variance (std 0.1 -> invstd ~ 10)
    assert 5.0 < float(on["st0"][1, 1]) < 20.0


@pytest.mark.parametrize("k", [3, 5])
def test_weight_gradient_bitwise_at_one_split(k):
    """C >= 512 (the 16x16 stages have 672 / 960): the separate weight-gradient kernel takes one
    split per channel, whose chain order the fused kernel repeats, so the depthwise weight
    gradient is bitwise equal too, on the 8-wave layout (N = 32) and the 4-wave one (N = 16)."""
    for N in (32, 16):
        on, off = _run(N, 516, k, 2), _run(N, 516, k, 1)
        for key in BITWISE + ["dw"]:
            assert torch.equal(on[key], off[key]), (N, key)


def test_too_large_batch_falls_back():
    """N = 33: 8448 elements per channel, e2ep_mbconv_mid_ok is 0, the entry points refuse the
    shape and the op runs the separate launches (equal outputs with the key on and off)."""
    from e2ep_amd import _lib
    N, C, K = 33, 3, 3
    d = _lib.dims((N, C, 16, 16, K, 16, 16, 1, 1, 1))
    assert _lib.load().e2ep_mbconv_mid_ok(d) == 0
    assert _lib.load().e2ep_mbconv_mid_fwd(*([None] * 2), d, *([None] * 4), 0.0, 0.0,
                                           *([None] * 5), 0.0, 0.0, *([None] * 4)) != 0
    on, off = _run(N, C, K, 2), _run(N, C, K, 1)
    for k in BITWISE + ["dw"]:
        assert torch.equal(on[k], off[k]), k
    ref = _ref64(N, C, K)
    for k in sorted(ref):
        print(f"N33 {k}: err {_err(on[k], ref[k]):.3e}")


def test_key_off_and_other_shapes_not_taken():
    from e2ep_amd import _lib
    ok = lambda *d: _lib.load().e2ep_mbconv_mid_ok(_lib.dims(d))  # noqa: E731
    assert ok(32, 960, 16, 16, 5, 16, 16, 1, 2, 2) == 1
    assert ok(32, 672, 16, 16, 3, 16, 16, 1, 1, 1) == 1
    assert ok(32, 336, 32, 32, 5, 32, 32, 1, 2, 2) == 0   # 32 x 32 maps
    assert ok(32, 336, 32, 32, 3, 16, 16, 2, 0, 0) == 0   # stride 2
    assert ok(8, 64, 16, 16, 3, 16, 16, 1, 0, 0) == 0     # not SAME padding
    assert ok(8, 64, 16, 16, 7, 16, 16, 1, 3, 3) == 0     # K = 7
    prev = _tune(KEY, 1)
    try:
        assert ok(32, 960, 16, 16, 5, 16, 16, 1, 2, 2) == 0
    finally:
        _tune(KEY, prev)


def test_running_statistics_after_two_calls():
    case = (5, 8, 3)
    on, off = _run(*case, 2, calls=2), _run(*case, 1, calls=2)
    for k in ("rm0", "rv0", "rm1", "rv1"):
        assert torch.equal(on[k], off[k]), k
    # float64: two updates with the same batch statistics, from mean 0 / var 1.  Bound: the
    # mean-100 channel's normalised values carry up to 100 * 2^-24 / 0.1 = 6e-5 relative error
    # from the fp32 mean, which reaches y1 and so _bn1's statistics; 1e-3 covers it.
    xc = _inputs(*case)[0].double()
    y1 = _ref64(*case)["y1"]
    for t, rm, rv in ((xc, "rm0", "rv0"), (y1, "rm1", "rv1")):
        m, v = t.mean((0, 2, 3)), t.var((0, 2, 3), unbiased=True)
        want_m = MOM * m * (1 + (1 - MOM))
        want_v = (1 - MOM) ** 2 + MOM * v * (1 + (1 - MOM))
        assert torch.allclose(on[rm].double().cpu(), want_m, rtol=1e-3, atol=1e-6), rm
        assert torch.allclose(on[rv].double().cpu(), want_v, rtol=1e-3, atol=1e-6), rv


def test_two_runs_bitwise_equal():
    case = (32, 8, 5)
    a, b = _run(*case, 2), _run(*case, 2)
    for k in BITWISE + ["dw"]:
        assert torch.equal(a[k], b[k]), k


def test_graph_replay_equals_eager():
    """Forward + backward captured with e2ep_amd.graphs.capture and replayed."""
    from e2ep_amd import graphs
    N, C, K = 5, 8, 3
    xc, gyc, p = _inputs(N, C, K)
    layers = _layers(C, K, p)
    x, gy = xc.to(DEV).requires_grad_(True), gyc.to(DEV)
    params = [q for m in layers for q in m.parameters()]

    def step():
        x.grad = None
        for q in params:
            q.grad = None
        y = _forward(x, layers)[0]
        y.backward(gy)
        return [y, x.grad] + [q.grad for q in params]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph, out, _ = graphs.capture(step)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(eager, out)):
        assert torch.equal(a, b), i


def _mbconv_ref64(blk, x, gy, u, keep, k):
    """float64 restatement of one MBConv block (training, skip + drop-connect)."""
    sd = {n: t.detach().double().cpu().requires_grad_(True) for n, t in blk.named_parameters()}
    x = x.detach().double().cpu().requires_grad_(True)
    bn = lambda t, n: F.batch_norm(t, None, None, sd[n + ".weight"], sd[n + ".bias"], True, 0.0, EPS)  # noqa: E731
    mid = sd["_depthwise_conv.weight"].shape[0]
    e = _swish(bn(F.conv2d(x, sd["_expand_conv.weight"]), "_bn0"))
    a1 = _swish(bn(F.conv2d(e, sd["_depthwise_conv.weight"], padding=k // 2, groups=mid), "_bn1"))
    h = _swish(F.conv2d(a1.mean((2, 3), keepdim=True), sd["_se_reduce.weight"], sd["_se_reduce.bias"]))
    a1 = a1 * torch.sigmoid(F.conv2d(h, sd["_se_expand.weight"], sd["_se_expand.bias"]))
    o = bn(F.conv2d(a1, sd["_project_conv.weight"]), "_bn2")
    o = o / keep * torch.floor(keep + u.double().cpu())[:, None, None, None] + x
    o.backward(gy.double().cpu())
    return sd["_depthwise_conv.weight"].grad


@pytest.mark.parametrize("k", [3, 5])
def test_mbconv_block_gradients(k):
    """One training MBConv block with a skip connection and drop-connect: the output, the input
    gradient and every parameter gradient, key on against key off."""
    from model.efficientnet import MBConv
    g = torch.Generator().manual_seed(k)
    x0 = torch.randn(4, 8, 16, 16, generator=g).to(DEV)
    gy = torch.randn(4, 8, 16, 16, generator=g).to(DEV)
    u = torch.tensor([0.9, 0.05, 0.5, 0.3], device=DEV)  # sample 1 is dropped at keep 0.8
    torch.manual_seed(k)
    blk = MBConv(8, 8, k, 1, 6, 16, False).to(DEV).train()
    res = {}
    for key in (2, 1):
        prev = _tune(KEY, key)
        try:
            blk.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_(True)
            out = blk(x, 0.2, u)
            out.backward(gy)
            torch.cuda.synchronize()
        finally:
            _tune(KEY, prev)
        res[key] = dict(out=out.detach().clone(), dx=x.grad.clone(),
                        **{n: q.grad.clone() for n, q in blk.named_parameters()})
    assert set(res[2]) == set(res[1]) and "_bn0.weight" in res[2]
    for n in res[2]:
        if n != "_depthwise_conv.weight":
            assert torch.equal(res[2][n], res[1][n]), n
    ref = _mbconv_ref64(blk, x0, gy, u, 0.8, k)
    e_on = _err(res[2]["_depthwise_conv.weight"], ref)
    e_off = _err(res[1]["_depthwise_conv.weight"], ref)
    print(f"MBConv k{k} depthwise weight gradient: fused err {e_on:.3e}, separate err {e_off:.3e}")
    assert e_on <= 2.0 * e_off
