"""The decoder and resize entry points of the C ABI at non-minimal ldx / ldkv / ldr / ldo /
seq_stride / x_nstride / y_nstride / g_pstride, on operands placed inside NaN- or
sentinel-filled parents (tests/placement.py), and the two nn_ops wrappers whose entry points
refuse pointers off 16-byte alignment.

e2ep_dec_row_gemv: against an fp64 reference written out below, at test_ar_decode_gpu's TOL.
e2ep_dec_cross_attn / e2ep_dec_self_attn: bitwise equal to the same entry point on dense copies
(test_ar_decode_gpu asserts those against fp64 through IncrementalDecoder).  e2ep_resize_fwd /
_bwd: against F.interpolate at test_resize's bounds (1e-6 vs fp32, 2e-5 vs fp64).  Every
output: no NaN, gaps untouched; every case under guard.allocations with both fills."""
import pytest
import torch
import torch.nn.functional as F

import guard
import placement as P
from helpers import rel_l2
from test_ar_decode_gpu import TOL, _module

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILLS = (guard.FILL_A, guard.FILL_B)


def _L():
    from e2ep_amd import _lib
    return _lib


def _dev(t, off=0):
    """A dense device copy of a host tensor `off` floats past an aligned address."""
    return P.placed(t, None, off, device=DEV) if off else guard.put(t, DEV)


# ------------------------------------------------------------------------------------------
# e2ep_dec_row_gemv
# ------------------------------------------------------------------------------------------
def _ln64(x, gamma, beta, eps):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)  # biased, as torch's LayerNorm
    return (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


@pytest.mark.parametrize("woff", [0, 1], ids=["w_al8", "w_off4"])
@pytest.mark.parametrize("K", [26, 27])
def test_dec_row_gemv_strided_rows(K, woff):
    """out[b][n] = act(LN?(x[b]) . w[n] + bias[n]) + LN?(res[b])[n] with ldx = K + 3,
    ldr = N + 2, ldo = N + 5; B = 5 crosses the 4-row chunk.  K = 26 with w 8-byte aligned runs
    k_dec_row_gemv<2>, every other case <1>."""
    L = _L()
    B, N, eps, reps = 5, 11, 1e-5, 1e-3
    g = torch.Generator().manual_seed(10 * K + woff)
    x, w, bias = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) / 4, torch.randn(N, generator=g)
    res = torch.randn(B, N, generator=g)
    gam, bet = 1 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    rgam, rbet = 1 + 0.2 * torch.randn(N, generator=g), 0.2 * torch.randn(N, generator=g)
    for fill in FILLS:
        with guard.allocations(fill) as gd:
            wd = _dev(w, woff)
            assert wd.data_ptr() % 8 == 4 * woff
            bd, gd_, bt_, rg_, rb_ = (_dev(t, 1) for t in (bias, gam, bet, rgam, rbet))
            xp = P.placed(x, K + 3, 1, device=DEV)
            rp = P.placed(res, N + 2, 3, device=DEV)
            for ln in (False, True):
                for rmode in ("none", "res", "res_ln"):
                    for relu in (False, True):
                        o = P.out((B, N), N + 5, 1, device=DEV)
                        has_res, has_rln = rmode != "none", rmode == "res_ln"
                        L.call("e2ep_dec_row_gemv", L.ptr(xp), K + 3, L.ptr(gd_ if ln else None),
                               L.ptr(bt_ if ln else None), eps, L.ptr(wd), L.ptr(bd),
                               L.ptr(rp if has_res else None), N + 2 if has_res else 0,
                               L.ptr(rg_ if has_rln else None), L.ptr(rb_ if has_rln else None), reps,
                               L.ptr(o), N + 5, B, N, K, int(relu), L.stream())
                        want = (_ln64(x, gam, bet, eps) if ln else x.double()) @ w.double().t() + bias.double()
                        if relu:
                            want = want.clamp_min(0)
                        if has_res:
                            want = want + (_ln64(res, rgam, rbet, reps) if has_rln else res.double())
                        what = f"K {K} woff {woff} ln {ln} {rmode} relu {relu}"
                        assert not bool(o.isnan().any()), what
                        err = rel_l2(o, want)
                        assert err < TOL, (what, err)
                        P.check_gaps(o, what)
        gd.check()


# ------------------------------------------------------------------------------------------
# e2ep_dec_cross_attn / e2ep_dec_self_attn
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sk", [5, 131])
@pytest.mark.parametrize("name", ["small", "odd"])
def test_dec_cross_attn_strided_rows_and_kv(name, Sk):
    L = _L()
    cp, _ = _module(name)
    layer = cp.tf_decoder.layers[1]
    ca, norm = layer.multihead_attn, layer.norm1
    E, H, B = cp.cfg.tf_de_dim, ca.num_heads, 3
    g = torch.Generator().manual_seed(Sk + E)
    x, kv = torch.randn(B, E, generator=g), torch.randn(B, Sk, 2 * E, generator=g)

    def run(xd, kvd, out):
        L.call("e2ep_dec_cross_attn", L.ptr(xd), xd.stride(0), L.ptr(norm.weight), L.ptr(norm.bias),
               norm.eps, L.ptr(ca.in_proj_weight), L.ptr(ca.in_proj_bias), L.ptr(kvd), kvd.stride(1),
               L.ptr(out), B, Sk, E, H, L.stream())
        return out
    dense = run(x.to(DEV), kv.to(DEV), torch.full((B, E), float("nan"), device=DEV))
    assert not bool(dense.isnan().any())
    for fill in FILLS:
        with guard.allocations(fill) as gd:
            xp = P.placed(x, E + 3, 1, device=DEV)
            kvp = P.placed(kv, 2 * E + 6, 3, device=DEV)
            assert kvp.stride() == (Sk * (2 * E + 6), 2 * E + 6, 1)
            out = run(xp, kvp, P.out((B, E), None, 1, device=DEV))
            assert torch.equal(out, dense)
            P.check_gaps(out, "cross-attention out")
        gd.check()


@pytest.mark.parametrize("t", [0, 3])
@pytest.mark.parametrize("name", ["small", "odd"])
def test_dec_self_attn_strided_rows_and_seq(name, t):
    """ldx = E + 1, seq_stride = T + 3 (gap tokens are PAD: a key read from a gap would be
    masked); the cache, written at position t, and the output sit one float off alignment."""
    L = _L()
    cp, _ = _module(name)
    layer = cp.tf_decoder.layers[1]
    sa, norm = layer.self_attn, cp.tf_decoder.layers[0].norm3
    E, H, B, T = cp.cfg.tf_de_dim, sa.num_heads, 3, cp.cfg.tf_de_tgt_dim - 1
    pad = cp.pad_idx
    g = torch.Generator().manual_seed(t + E)
    x = torch.randn(B, E, generator=g)
    cache0 = torch.full((B, T, 2, E), float("nan"))
    cache0[:, :t] = torch.randn(B, t, 2, E, generator=g)
    seq = torch.full((B, T), pad, dtype=torch.long)
    seq[:, :t + 1] = torch.randint(0, pad, (B, t + 1), generator=g)

    def run(xd, seqd, cache, out):
        L.call("e2ep_dec_self_attn", L.ptr(xd), xd.stride(0), L.ptr(norm.weight), L.ptr(norm.bias),
               norm.eps, None, 0, None, None, L.ptr(seqd), seqd.stride(0), pad,
               L.ptr(sa.in_proj_weight), L.ptr(sa.in_proj_bias), L.ptr(cache), L.ptr(out), B, T, t, E,
               H, L.stream())
        return cache, out
    dcache, dout = run(x.to(DEV), seq.to(DEV), cache0.to(DEV), torch.full((B, E), float("nan"), device=DEV))
    assert not bool(dout.isnan().any()) and not bool(dcache[:, :t + 1].isnan().any())
    assert bool(dcache[:, t + 1:].isnan().all())  # later positions stay unwritten
    for fill in FILLS:
        with guard.allocations(fill) as gd:
            xp = P.placed(x, E + 1, 3, device=DEV)
            sp = P.placed(seq, T + 3, 1, fill=pad, device=DEV)
            cache = P.placed(cache0, None, 1, fill=P.SENTINEL, device=DEV)
            cache, out = run(xp, sp, cache, P.out((B, E), None, 1, device=DEV))
            assert torch.equal(out, dout)
            assert torch.equal(cache[:, :t + 1], dcache[:, :t + 1])
            assert bool(cache[:, t + 1:].isnan().all())
            P.check_gaps(out, "self-attention out")
            P.check_gaps(cache, "self-attention cache")
            P.check_gaps(sp, "seq")
        gd.check()


# ------------------------------------------------------------------------------------------
# e2ep_resize_fwd / e2ep_resize_bwd
# ------------------------------------------------------------------------------------------
RESIZE = [((2, 5, 17, 9), (40, 8)), ((2, 5, 17, 9), (40, 7))]


@pytest.mark.parametrize("shape,size", RESIZE, ids=["Wo8_vector", "Wo7_scalar"])
def test_resize_fwd_channel_slices(shape, size):
    """x and y are channel slices [1 : 1 + C] of wider tensors: x_nstride = (C + 2) Hi Wi,
    y_nstride = (C + 3) Ho Wo.  Wo = 8 takes k_resize_fwd4 (y 16-byte aligned, y_nstride % 4
    == 0), Wo = 7 the scalar kernel."""
    L = _L()
    N, C, Hi, Wi = shape
    Ho, Wo = size
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(Wo))
    y32 = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    y64 = F.interpolate(x.double(), size=size, mode="bilinear", align_corners=False)
    xs = ((C + 2) * Hi * Wi, Hi * Wi, Wi, 1)
    ys = ((C + 3) * Ho * Wo, Ho * Wo, Wo, 1)
    for fill in FILLS:
        with guard.allocations(fill) as gd:
            xp = P.placed(x, off=Hi * Wi, strides=xs, device=DEV)
            y = P.out((N, C, Ho, Wo), off=Ho * Wo, strides=ys, device=DEV)
            assert (Wo % 4 == 0 and ys[0] % 4 == 0 and y.data_ptr() % 16 == 0) == (Wo == 8)
            L.call("e2ep_resize_fwd", L.ptr(xp), N, C, xs[0], Hi, Wi, Ho, Wo, Hi / Ho, Wi / Wo,
                   L.ptr(y), ys[0], L.stream())
            assert not bool(y.isnan().any())
            e32, e64 = rel_l2(y, y32), rel_l2(y, y64)
            print(f"resize_fwd {shape} -> {size}: rel-L2 vs fp32 {e32:.3e}, vs fp64 {e64:.3e}")
            assert e32 < 1e-6 and e64 < 2e-5
            P.check_gaps(y, "resize_fwd y")
        gd.check()


@pytest.mark.parametrize("shape,size", RESIZE, ids=["Wo8", "Wo7"])
def test_resize_bwd_plane_stride(shape, size):
    """g_pstride = Ho Wo + 5 with g three floats off alignment; gx one float off."""
    L = _L()
    N, C, Hi, Wi = shape
    Ho, Wo = size
    planes = N * C
    gen = torch.Generator().manual_seed(Wo + 1)
    g = torch.randn(N, C, Ho, Wo, generator=gen)
    want = []
    for dt in (torch.float32, torch.float64):
        x = torch.zeros(*shape, dtype=dt, requires_grad=True)
        F.interpolate(x, size=size, mode="bilinear", align_corners=False).backward(g.to(dt))
        want.append(x.grad.view(planes, Hi * Wi))
    for fill in FILLS:
        with guard.allocations(fill) as gd:
            gp = P.placed(g.view(planes, Ho * Wo), Ho * Wo + 5, 3, device=DEV)
            gx = P.out((planes, Hi * Wi), None, 1, device=DEV)
            ws = torch.empty(max(16, L.load().e2ep_resize_bwd_workspace(planes, Ho, Wi)),
                             dtype=torch.uint8, device=DEV)
            L.call("e2ep_resize_bwd", L.ptr(gp), Ho * Wo + 5, planes, Hi, Wi, Ho, Wo, Hi / Ho, Wi / Wo,
                   L.ptr(gx), 0, L.ptr(ws), L.stream())
            assert not bool(gx.isnan().any())
            e32, e64 = rel_l2(gx, want[0]), rel_l2(gx, want[1])
            print(f"resize_bwd {shape} <- {size}: rel-L2 vs fp32 {e32:.3e}, vs fp64 {e64:.3e}")
            assert e32 < 1e-6 and e64 < 2e-5
            P.check_gaps(gx, "resize_bwd gx")
        gd.check()


# ------------------------------------------------------------------------------------------
# nn_ops.relu_dropout / nn_ops.cat_channels on tensors 4 bytes off 16-byte alignment
# ------------------------------------------------------------------------------------------
def _off4(t):
    """A dense device copy of `t` with data_ptr() % 16 == 4: flat[1 : 1 + n].view(shape)."""
    flat = torch.full((t.numel() + 4,), float("nan"), device=DEV)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_relu_dropout_accepts_misaligned_tensors(p):
    from e2ep_amd import nn_ops
    L = _L()
    gen = torch.Generator().manual_seed(3)
    x, dy = torch.randn(6, 10, 14, generator=gen), torch.randn(6, 10, 14, generator=gen)
    seed = torch.tensor([12345], dtype=torch.int32, device=DEV)
    outs = []
    for mis in (False, True):
        xd = (_off4(x) if mis else x.to(DEV)).requires_grad_()
        y = nn_ops.relu_dropout(xd, p, seed)
        y.backward(_off4(dy) if mis else dy.to(DEV))
        outs.append((y.detach(), xd.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    want = x.clamp_min(0)
    kept = outs[0][0].cpu() != 0
    if p == 0.0:
        assert torch.equal(outs[0][0].cpu(), want)
    else:
        assert 0.55 < float(kept[want > 0].float().mean()) < 0.85  # about 1 - p survive
    # the entry point itself keeps its refusal
    xm, ya = _off4(x), torch.empty(x.numel(), device=DEV)
    rc = L.call_raw("e2ep_relu_dropout_fwd", L.ptr(xm), x.numel(), 0.0, None, L.ptr(ya), L.stream())
    assert rc == L.CONSTANTS["E2EP_EINVAL"] and b"16-B aligned" in L.load().e2ep_last_error()


def test_cat_channels_accepts_misaligned_tensors():
    from e2ep_amd import nn_ops
    gen = torch.Generator().manual_seed(4)
    a, b = torch.randn(2, 3, 4, 6, generator=gen), torch.randn(2, 5, 4, 6, generator=gen)
    g = torch.randn(2, 8, 4, 6, generator=gen)
    outs = []
    for mis in (False, True):
        ad = (_off4(a) if mis else a.to(DEV)).requires_grad_()
        bd = b.to(DEV).requires_grad_()
        y = nn_ops.cat_channels([ad, bd])
        y.backward(_off4(g) if mis else g.to(DEV))
        outs.append((y.detach(), ad.grad, bd.grad))
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    assert torch.equal(outs[1][0].cpu(), torch.cat([a, b], 1))
    assert torch.equal(outs[1][1].cpu(), g[:, :3]) and torch.equal(outs[1][2].cpu(), g[:, 3:])
