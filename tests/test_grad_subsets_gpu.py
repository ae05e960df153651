"""Every autograd op with some of its inputs frozen, and with its optional parameters absent.

The rest of the suite gives every input requires_grad=True and builds every BatchNorm2d /
LayerNorm affine with running statistics, so the null-output branches of the kernels
(`if (dx)`, `if (dgamma)`, k_bn_bwd_finalize, ...), the needs_input_grad branches of the
wrappers (pair launch or fork, e2ep_gemm_rowsum / e2ep_gemm / e2ep_col_sum, which slot of the
returned tuple holds which gradient) and the `gamma ? gamma[c] : 1.f` reads never run there.

One case = one op at one shape (`Case`): its float inputs (`leaves`), constants, the call and an
fp64 CPU restatement in plain torch.  For a subset S of the leaves `check` runs the op in
guard-banded, poisoned buffers (tests/guard.py) under both fills with exactly S requiring a
gradient and asserts

  (a) the forward outputs (and BatchNorm running statistics) are bitwise those of the run in
      which every leaf requires a gradient,
  (b) every gradient in S is within the bound of the op's existing fp64 test (the bounds are
      copied from the tests named beside them; none is new),
  (c) every gradient in S is bitwise the all-gradients run's, except where the subset really
      runs other arithmetic (listed at the case, and in DESIGN.md section 8),
  (d) every leaf outside S has .grad None, no guard band was written, and the two fills give
      the same bits (poison in a result would differ between them).

The fp64 reference is computed once per case and shared by its subsets."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import guard
from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILLS = (guard.FILL_A, guard.FILL_B)
EPS, MOM = 1e-3, 0.01  # efficientnet-pytorch's BatchNorm settings, as the existing BN tests


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _swish(z):
    return z * torch.sigmoid(z)


# ----------------------------------------------------------------------------------------------
# the engine
# ----------------------------------------------------------------------------------------------
class Case:
    """leaves / consts: name -> CPU tensor (fp32 leaves; constants of any dtype).  gys: the
    gradients fed to the outputs.  fn(t, c) and ref(t, c) take the leaves as Parameters and the
    constants (on the device in fp32 for fn, on the CPU in fp64 for ref) and return
    (outputs, aux): a tuple of differentiable outputs and a dict of other results (running
    statistics).  bounds: 'y' (or 'y0', 'y1'), every leaf and every aux name -> rel-L2 bound.
    key: the case without its kernel-route settings (the fp64 reference is shared over them).
    ref_leaves / ref_gys: what the reference is given instead (operands rounded to bf16)."""

    def __init__(self, key, leaves, consts, gys, fn, ref, bounds, settings=(), ref_leaves=None,
                 ref_gys=None):
        self.key, self.leaves, self.consts, self.gys = key, leaves, consts, gys
        self.fn, self.ref, self.bounds, self.settings = fn, ref, bounds, settings
        self.ref_leaves, self.ref_gys = ref_leaves or leaves, ref_gys or gys
        self._full = None

    def bound(self, name, i=0):
        return self.bounds[name] if name in self.bounds else self.bounds[f"y{i}"]


class Run:
    def __init__(self, ys, aux, grads, pending):
        self.ys, self.aux, self.grads, self.pending = ys, aux, grads, pending


_REF = {}


def _ref(case):
    """The fp64 CPU result of the case with every leaf requiring a gradient, computed once."""
    if case.key not in _REF:
        t = {k: nn.Parameter(v.double()) for k, v in case.ref_leaves.items()}
        c = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in case.consts.items()}
        ys, aux = case.ref(t, c)
        torch.autograd.backward(list(ys), [g.double() for g in case.ref_gys])
        _REF[case.key] = Run([y.detach() for y in ys], {k: v.detach() for k, v in aux.items()},
                             {k: p.grad for k, p in t.items()}, None)
    return _REF[case.key]


def _run(case, need, fill, scoped=False):
    """One forward + backward in guarded buffers with exactly the leaves in `need` requiring a
    gradient; scoped: inside a defer.ParamGradDefer scope (pending = the records it held just
    before its flush)."""
    from e2ep_amd import _lib, defer
    pending = None
    with contextlib.ExitStack() as st:
        for s in case.settings:
            st.enter_context(s())
        g = st.enter_context(guard.allocations(fill))
        t = {k: nn.Parameter(guard.put(v), requires_grad=k in need) for k, v in case.leaves.items()}
        c = {k: guard.put(v) for k, v in case.consts.items()}
        gys = [guard.put(v) for v in case.gys]
        with (defer.ParamGradDefer() if scoped else contextlib.nullcontext()):
            ys, aux = case.fn(t, c)
            live = [(y, gy) for y, gy in zip(ys, gys) if y.requires_grad]
            torch.autograd.backward([y for y, _ in live], [gy for _, gy in live])
            if scoped:
                pending = _lib.call_raw("e2ep_defer_pending")
        if scoped:
            assert _lib.call_raw("e2ep_defer_pending") == 0
        torch.cuda.synchronize()
        out = Run([y.detach().cpu() for y in ys], {k: v.detach().cpu() for k, v in aux.items()},
                  {k: (None if p.grad is None else p.grad.cpu()) for k, p in t.items()}, pending)
        g.check()
    return out


def _full(case):
    """The guarded run with every leaf requiring a gradient (once per case); its forward is
    held to the fp64 bound here, its gradients by the op's existing test."""
    if case._full is None:
        case._full = _run(case, set(case.leaves), guard.FILL_A)
        ref = _ref(case)
        for i, (y, y64) in enumerate(zip(case._full.ys, ref.ys)):
            assert rel_l2(y, y64) < case.bound("y", i), f"forward output {i}"
    return case._full


def _check_grads(case, r, ref, names, tag):
    for k in names:
        assert r.grads[k] is not None, f"{tag}: no gradient for {k}"
        e = rel_l2(r.grads[k], ref.grads[k])
        print(f"{tag} d{k}: rel-L2 vs fp64 {e:.3e} (bound {case.bounds[k]:.0e})")
        assert e < case.bounds[k], f"{tag}: d{k} {e:.3e}"                              # (b)


def check(case, need, inexact=(), scoped=False):
    """(a) - (d) of the module docstring for the subset `need`; inexact: the gradients that the
    subset forms with other arithmetic than the all-gradients run ((b) only)."""
    need = set(need)
    assert need <= set(case.leaves), need - set(case.leaves)
    full, ref = _full(case), _ref(case)
    runs = [_run(case, need, fill, scoped) for fill in FILLS]
    for fill, r in zip(FILLS, runs):
        tag = f"fill 0x{fill:02X}"
        assert len(r.ys) == len(full.ys)
        for i, (a, b) in enumerate(zip(r.ys, full.ys)):
            assert torch.equal(a, b), f"{tag}: forward output {i} differs"             # (a)
        for k, v in full.aux.items():
            assert torch.equal(r.aux[k], v), f"{tag}: {k} differs"
        _check_grads(case, r, ref, sorted(need), tag)
        for k in case.leaves:
            if k not in need:
                assert r.grads[k] is None, f"{tag}: frozen {k} got a gradient"         # (d)
            elif k not in inexact:
                assert torch.equal(r.grads[k], full.grads[k]), f"{tag}: d{k} differs from the all-gradients run"  # (c)
            else:
                print(f"{tag} d{k}: other arithmetic than the all-gradients run, bitwise equal: "
                      f"{torch.equal(r.grads[k], full.grads[k])}")
    for k in need:
        assert torch.equal(runs[0].grads[k], runs[1].grads[k]), f"d{k} depends on the fill"
    return runs


def check_full(case):
    """A case with absent parameters: outputs, running statistics and every gradient against
    the fp64 module built the same way, in guarded buffers under both fills."""
    ref = _ref(case)
    runs = [_run(case, set(case.leaves), fill) for fill in FILLS]
    for fill, r in zip(FILLS, runs):
        tag = f"fill 0x{fill:02X}"
        for i, (y, y64) in enumerate(zip(r.ys, ref.ys)):
            assert rel_l2(y, y64) < case.bound("y", i), f"{tag}: forward output {i}"
        for k, v in ref.aux.items():
            assert rel_l2(r.aux[k], v) < case.bounds[k], f"{tag}: {k}"
        _check_grads(case, r, ref, sorted(case.leaves), tag)
    for a, b in zip(runs[0].ys + list(runs[0].grads.values()), runs[1].ys + list(runs[1].grads.values())):
        assert torch.equal(a, b), "a result depends on the fill"
    return runs


@contextlib.contextmanager
def _bn_small(on):
    """1: channels of N*H*W <= 32768 on the single-launch kernels; 0: every shape on the split
    reduce + apply kernels (test_nn_ops_gpu.py's bn_path)."""
    from e2ep_amd import _lib
    prev = _lib.call_raw("e2ep_bn_small", int(on))
    try:
        yield
    finally:
        _lib.call_raw("e2ep_bn_small", prev)


@contextlib.contextmanager
def _se_bn_sums(on):
    from e2ep_amd import nn_ops
    prev = nn_ops.set_se_bn_sums(on)
    try:
        yield
    finally:
        nn_ops.set_se_bn_sums(prev)


def _bn(C, t, c, train, affine=True, track=True, pre=""):
    """BatchNorm2d over the case's tensors (device fp32 or CPU fp64 alike)."""
    bn = nn.BatchNorm2d(C, momentum=MOM, eps=EPS, affine=affine, track_running_stats=track)
    if affine:
        bn.weight, bn.bias = t[pre + "gamma"], t[pre + "beta"]
    if track:
        bn.running_mean, bn.running_var = c[pre + "rm"], c[pre + "rv"]
        bn.num_batches_tracked = torch.zeros((), dtype=torch.long, device=c[pre + "rm"].device)
    return bn.train(train)


def _bn_aux(bn, pre=""):
    if not bn.track_running_stats:
        return {}
    return {pre + "rm": bn.running_mean, pre + "rv": bn.running_var}


def _bn_tensors(C, g, affine, track, pre=""):
    """(leaves, consts) of one BatchNorm, drawn as test_nn_ops_gpu.py's test_bn_act draws them."""
    leaves, consts = {}, {}
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    rm, rv = 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    if affine:
        leaves[pre + "gamma"], leaves[pre + "beta"] = gamma, beta
    if track:
        consts[pre + "rm"], consts[pre + "rv"] = rm, rv
    return leaves, consts


def _ids(subsets):
    return ["+".join(s) for s in subsets]


# ----------------------------------------------------------------------------------------------
# batch_norm_act
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bn_case(shape, small, act, res, dc, train, affine=True, track=True):
    N, C, H, W = shape
    g = _g(sum(shape) + 3 * train)
    leaves = {"x": torch.randn(*shape, generator=g) * 2 + 0.5}
    bl, consts = _bn_tensors(C, g, affine, track)
    leaves.update(bl)
    if res:
        leaves["res"] = torch.randn(*shape, generator=g)
    keep = 0.8
    u = torch.rand(N, generator=g)
    u[0], u[1] = 0.05, 0.9  # sample 0 is dropped at keep 0.8, sample 1 kept
    if dc:
        consts["u"] = u
        assert 0 < torch.floor(keep + u).sum() < N  # kept and dropped samples
    gy = torch.randn(*shape, generator=g)

    def fn(t, c):
        from e2ep_amd import nn_ops
        bn = _bn(C, t, c, train, affine, track)
        y = nn_ops.batch_norm_act(t["x"], bn, act, t.get("res"), dc_rand=c.get("u"),
                                  dc_keep=keep if dc else 1.0)
        return (y,), _bn_aux(bn)

    def ref(t, c):
        bn = _bn(C, t, c, train, affine, track)
        z = bn(t["x"])
        if dc:  # efficientnet-pytorch drop_connect, the mask formed in fp32 as the kernel does
            z = z / keep * torch.floor(torch.tensor(keep, dtype=torch.float32) + u).double().view(N, 1, 1, 1)
        if res:
            z = z + t["res"]
        return (_swish(z) if act == "swish" else z,), _bn_aux(bn)

    # test_nn_ops_gpu.py test_bn_act / test_bn_drop_connect_fused
    bounds = dict(y=1e-6, x=1e-5, gamma=1e-5, beta=1e-5, res=1e-6, rm=1e-6, rv=1e-6)
    return Case(("bn", shape, act, res, dc, train, affine, track), leaves, consts, [gy], fn, ref,
                bounds, (lambda: _bn_small(small),))


BN_SHAPES = [(3, 7, 5, 9), (4, 24, 16, 16)]
# id -> (act, residual, drop-connect, train)
BN_CONFIGS = {"none": (None, False, False, True), "swish": ("swish", False, False, True),
              "none_res": (None, True, False, True), "swish_res": ("swish", True, False, True),
              "none_res_dropconnect": (None, True, True, True),
              "none_eval": (None, False, False, False), "swish_res_eval": ("swish", True, False, False)}
BN_SUBSETS = [("x",), ("gamma", "beta"), ("res",), ("x", "res"), ("gamma",)]
BN_PARAMS = [pytest.param(cfg, s, id=f"{cfg}-{'+'.join(s)}") for cfg in BN_CONFIGS for s in BN_SUBSETS
             if BN_CONFIGS[cfg][1] or "res" not in s]


@pytest.mark.parametrize("small", [1, 0], ids=["bn_one_launch", "bn_split"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=["3x7x5x9", "4x24x16x16"])
@pytest.mark.parametrize("cfg,subset", BN_PARAMS)
def test_batch_norm_act(cfg, subset, shape, small):
    """(3,7,5,9) takes the split route under both settings (H*W is no multiple of 4),
    (4,24,16,16) k_bn_bwd_small or the split route.  On the split route {gamma, beta} and
    {gamma} end in k_bn_bwd_finalize instead of k_bn_bwd_apply: both take the channel sums
    from channel_partials() and round them to fp32 the same way, so (c) holds bitwise."""
    check(bn_case(shape, small, *BN_CONFIGS[cfg]), subset)


# ----------------------------------------------------------------------------------------------
# depthwise_conv2d, bn_act_depthwise_conv2d
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dw_case(dims, fused, small=1, train=True, affine=True, track=True):
    N, C, H, W, K, s, pad = dims
    g = _g(C + H + K)
    leaves = {"x": torch.randn(N, C, H, W, generator=g) * 2 + 0.5,
              "w": torch.randn(C, 1, K, K, generator=g) / K}
    consts = {}
    if fused:
        bl, consts = _bn_tensors(C, g, affine, track)
        leaves.update(bl)
    P, Q = (H + pad[2] + pad[3] - K) // s + 1, (W + pad[0] + pad[1] - K) // s + 1
    gy = torch.randn(N, C, P, Q, generator=g)

    def fn(t, c):
        from e2ep_amd import nn_ops
        if not fused:
            return (nn_ops.depthwise_conv2d(t["x"], t["w"], s, pad),), {}
        bn = _bn(C, t, c, train, affine, track)
        return (nn_ops.bn_act_depthwise_conv2d(t["x"], bn, "swish", t["w"], s, pad),), _bn_aux(bn)

    def ref(t, c):
        z, aux = t["x"], {}
        if fused:
            bn = _bn(C, t, c, train, affine, track)
            z = _swish(bn(z))
            aux = _bn_aux(bn)
        return (F.conv2d(F.pad(z, pad), t["w"], None, s, 0, 1, C),), aux

    if fused:  # test_nn_ops_gpu.py test_bn_swish_depthwise_fused
        bounds = dict(y=1e-6, x=1e-5, w=1e-5, gamma=1e-5, beta=1e-5, rm=1e-6, rv=1e-6)
    else:      # test_nn_ops_gpu.py _depthwise_case (test_depthwise)
        bounds = dict(y=1e-6, x=1e-6, w=1e-5)
    return Case(("dw", dims, fused, train, affine, track), leaves, consts, [gy], fn, ref, bounds,
                (lambda: _bn_small(small),))


DW_DIMS = [(3, 16, 16, 16, 3, 1, (1, 1, 1, 1)), (3, 8, 13, 11, 3, 2, (0, 1, 0, 1))]
DW_IDS = ["s1_pairable", "s2"]
XW_SUBSETS = [("x",), ("w",)]


@pytest.mark.parametrize("dims", DW_DIMS, ids=DW_IDS)
@pytest.mark.parametrize("subset", XW_SUBSETS, ids=_ids(XW_SUBSETS))
def test_depthwise_conv2d(subset, dims):
    """The stride-1 shape's all-gradients run is one k_dw_bwd_pair launch, a subset the data or
    the weight gradient kernel alone: bitwise equal (test_depthwise_bwd_pair_bitwise_equals_
    two_launches)."""
    check(dw_case(dims, False), subset)


DW_FUSED_SUBSETS = [("x",), ("gamma", "beta"), ("w",), ("x", "w"), ("gamma", "beta", "w")]


@pytest.mark.parametrize("small", [1, 0], ids=["bn_one_launch", "bn_split"])
@pytest.mark.parametrize("dims", DW_DIMS, ids=DW_IDS)
@pytest.mark.parametrize("subset", DW_FUSED_SUBSETS, ids=_ids(DW_FUSED_SUBSETS))
def test_bn_act_depthwise_conv2d(subset, dims, small):
    """{w} alone launches no BN backward at all (no data gradient either): only dw comes back.
    {gamma, beta}: the data gradient kernel alone, then e2ep_bn_bwd without dx
    (k_bn_bwd_finalize on the split route)."""
    check(dw_case(dims, True, small), subset)


# ----------------------------------------------------------------------------------------------
# squeeze_excite, bn_swish_squeeze_excite
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def se_case(shape, fused, small=1, sums=True, bias=True, train=True, affine=True, track=True):
    N, C, H, W, sq = shape
    g = _g(C + sq + H)
    x = torch.randn(N, C, H, W, generator=g)
    leaves = {"x": x * 2 + 0.5 if fused else x,
              "w1": torch.randn(sq, C, 1, 1, generator=g) / C ** 0.5,
              "b1": torch.randn(sq, generator=g) * 0.1,
              "w2": torch.randn(C, sq, 1, 1, generator=g) / sq ** 0.5,
              "b2": torch.randn(C, generator=g) * 0.1}
    if not bias:
        del leaves["b1"], leaves["b2"]
    consts = {}
    if fused:
        bl, consts = _bn_tensors(C, g, affine, track)
        leaves.update(bl)
    gy = torch.randn(N, C, H, W, generator=g)

    def fn(t, c):
        from e2ep_amd import nn_ops
        se = (t["w1"], t.get("b1"), t["w2"], t.get("b2"))
        if not fused:
            return (nn_ops.squeeze_excite(t["x"], *se),), {}
        bn = _bn(C, t, c, train, affine, track)
        return (nn_ops.bn_swish_squeeze_excite(t["x"], bn, *se),), _bn_aux(bn)

    def ref(t, c):
        u, aux = t["x"], {}
        if fused:
            bn = _bn(C, t, c, train, affine, track)
            u = _swish(bn(u))
            aux = _bn_aux(bn)
        h = F.conv2d(F.adaptive_avg_pool2d(u, 1), t["w1"], t.get("b1"))
        a = F.conv2d(_swish(h), t["w2"], t.get("b2"))
        return (u * torch.sigmoid(a),), aux

    # test_nn_ops_gpu.py test_squeeze_excite_fused / test_bn_swish_se_fused
    bounds = dict(y=1e-6, x=1e-5, w1=1e-5, b1=1e-5, w2=1e-5, b2=1e-5, gamma=1e-5, beta=1e-5,
                  rm=1e-6, rv=1e-6)
    return Case(("se", shape, fused, bias, train, affine, track), leaves, consts, [gy], fn, ref,
                bounds, (lambda: _bn_small(small), lambda: _se_bn_sums(sums)))


SE_SHAPES = [(4, 40, 9, 7, 10), (8, 96, 16, 16, 6)]
SE_IDS = ["4x40x9x7", "8x96x16x16"]
SE_PARAMS = ("w1", "b1", "w2", "b2")
SE_SUBSETS = [("x",), SE_PARAMS, ("w2",)]
SE_NOBIAS_SUBSETS = [("x",), ("w1", "w2"), ("w2",)]
SE_FUSED_SUBSETS = SE_SUBSETS + [("gamma", "beta")]


@pytest.mark.parametrize("shape", SE_SHAPES, ids=SE_IDS)
@pytest.mark.parametrize("subset", SE_SUBSETS, ids=_ids(SE_SUBSETS))
def test_squeeze_excite(subset, shape):
    check(se_case(shape, False), subset)


@pytest.mark.parametrize("shape", SE_SHAPES, ids=SE_IDS)
@pytest.mark.parametrize("subset", SE_NOBIAS_SUBSETS, ids=_ids(SE_NOBIAS_SUBSETS))
def test_squeeze_excite_without_biases(subset, shape):
    """b1 = b2 = None: the `b1 ? b1[k] : 0.f` reads of the forward, no db1 / db2 buffers."""
    check(se_case(shape, False, bias=False), subset)


def _se_route_changes(shape, small, sums, subset):
    """True when the all-gradients run takes e2ep_se_bwd_bn + e2ep_bn_bwd_planes (a training
    BN on the split route, the sums wanted) and the subset, with x frozen, cannot."""
    from e2ep_amd import _lib
    with _bn_small(small):
        split = _lib.load().e2ep_bn_bwd_split(*shape[:4]) == 1
    return split and sums and "x" not in subset


@pytest.mark.parametrize("sums", [True, False], ids=["bn_sums_in_se", "bn_own_reduce"])
@pytest.mark.parametrize("small", [1, 0], ids=["bn_one_launch", "bn_split"])
@pytest.mark.parametrize("shape", SE_SHAPES, ids=SE_IDS)
@pytest.mark.parametrize("subset", SE_FUSED_SUBSETS, ids=_ids(SE_FUSED_SUBSETS))
def test_bn_swish_squeeze_excite(subset, shape, small, sums):
    """(4,40,9,7) is on the split BN route under both settings, (8,96,16,16) only with
    e2ep_bn_small off.  There, with the sums wanted, the all-gradients run is e2ep_se_bwd_bn +
    e2ep_bn_bwd_planes, which needs dx: a subset with x frozen must leave that route for
    e2ep_se_bwd + e2ep_bn_bwd (the `dx is not None` guard of _BnSwishSE.backward).  The two
    routes differ in arithmetic, not only in order: k_se_da<true> forms the SE input as
    (xhat gamma + beta) sigmoid(.) and sums it with the four BN terms, k_se_da<false> as
    swish(x scale + shift); da, and with it every SE parameter gradient and dpooled, differ in
    the last bits, and dgamma / dbeta come from the per-plane sums instead of
    k_bn_bwd_reduce's.  Those cases keep (b) only (test_bn_swish_se_fused holds both routes to
    the same fp64 bound)."""
    inexact = subset if _se_route_changes(shape, small, sums, subset) else ()
    check(se_case(shape, True, small, sums), subset, inexact)


# ----------------------------------------------------------------------------------------------
# mbconv_mid
# ----------------------------------------------------------------------------------------------
MID = (8, 96, 3, 4)  # N, C, K, sq on 16x16 maps
MID_PAD = (1, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def mid_case(fused, affine=True, track=True):
    N, C, K, sq = MID
    g = _g(1000 * N + 10 * C + K)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    leaves = {"x": r(N, C, 16, 16) * 2 + 0.5, "w": r(C, 1, K, K) / K, "w1": r(sq, C, 1, 1) / C ** 0.5,
              "b1": 0.1 * r(sq), "w2": r(C, sq, 1, 1) / sq ** 0.5, "b2": 0.1 * r(C)}
    consts = {}
    for pre in ("0.", "1."):
        bl, bc = _bn_tensors(C, g, affine, track, pre)
        leaves.update(bl)
        consts.update(bc)
    gy = r(N, C, 16, 16)

    def fn(t, c):
        from e2ep_amd import nn_ops
        bn0, bn1 = (_bn(C, t, c, True, affine, track, pre) for pre in ("0.", "1."))
        se = (t["w1"], t["b1"], t["w2"], t["b2"])
        if fused:
            assert nn_ops.mbconv_mid_ok(t["x"].shape, t["x"].dtype, bn0, bn1, t["w"], 1, MID_PAD)
            y = nn_ops.mbconv_mid(t["x"], bn0, t["w"], 1, MID_PAD, bn1, *se)
        else:
            y1 = nn_ops.bn_act_depthwise_conv2d(t["x"], bn0, "swish", t["w"], 1, MID_PAD, bn_stats=True)
            y = nn_ops.bn_swish_squeeze_excite(y1, bn1, *se)
        return (y,), {**_bn_aux(bn0, "0."), **_bn_aux(bn1, "1.")}

    def ref(t, c):
        bn0, bn1 = (_bn(C, t, c, True, affine, track, pre) for pre in ("0.", "1."))
        y1 = F.conv2d(_swish(bn0(t["x"])), t["w"], padding=K // 2, groups=C)
        u = _swish(bn1(y1))
        h = F.conv2d(F.adaptive_avg_pool2d(u, 1), t["w1"], t["b1"])
        a = F.conv2d(_swish(h), t["w2"], t["b2"])
        return (u * torch.sigmoid(a),), {**_bn_aux(bn0, "0."), **_bn_aux(bn1, "1.")}

    # the bounds of the two ops it replaces: test_nn_ops_gpu.py test_bn_swish_depthwise_fused and
    # test_bn_swish_se_fused (test_mbconv_mid_gpu.py itself compares with those ops bitwise)
    bounds = {k: 1e-5 for k in leaves}
    bounds.update({"y": 1e-6, "0.rm": 1e-6, "0.rv": 1e-6, "1.rm": 1e-6, "1.rv": 1e-6})
    return Case(("mid", affine, track), leaves, consts, [gy], fn, ref, bounds)


def _max_err(t, ref):
    """test_mbconv_mid_gpu.py's _err: max |t - ref| / max |ref|"""
    return float((t.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _mid_vs_separate(fused_runs, need, affine=True, track=True):
    """The fused op against bn_act_depthwise_conv2d + bn_swish_squeeze_excite with the same
    subset: bitwise, as e2ep.h promises ("every output is bitwise that of the separate
    launches"), except dw below 512 channels ("the same terms in another fixed order"), which
    is held to test_fused_equals_separate's bound: at most twice the separate path's own error
    against fp64."""
    sep_case = mid_case(False, affine, track)
    sep = _run(sep_case, need, guard.FILL_A)
    got, ref = fused_runs[0], _ref(sep_case)
    assert torch.equal(got.ys[0], sep.ys[0])
    for k, v in sep.aux.items():
        assert torch.equal(got.aux[k], v), k
    for k in sep_case.leaves:
        if k not in need:
            assert sep.grads[k] is None, k
        elif k != "w":
            assert torch.equal(got.grads[k], sep.grads[k]), f"d{k} differs from the separate launches"
    if "w" in need:
        e_on, e_off = _max_err(got.grads["w"], ref.grads["w"]), _max_err(sep.grads["w"], ref.grads["w"])
        print(f"depthwise weight gradient: fused err {e_on:.3e}, separate err {e_off:.3e}")
        assert e_on <= 2.0 * e_off


MID_FROZEN = {"x_frozen": ("x",), "bn0_frozen": ("0.gamma", "0.beta"), "bn1_frozen": ("1.gamma", "1.beta"),
              "dw_weight_frozen": ("w",), "se_frozen": SE_PARAMS}


@pytest.mark.parametrize("frozen", list(MID_FROZEN))
def test_mbconv_mid(frozen):
    """e2ep_mbconv_mid_bwd always forms dx and dw (the wrapper drops them) and takes the four BN
    gradients as nullable pointers; the SE parameter gradients come from e2ep_se_bwd."""
    case = mid_case(True)
    need = set(case.leaves) - set(MID_FROZEN[frozen])
    runs = check(case, need)
    _mid_vs_separate(runs, need)


# ----------------------------------------------------------------------------------------------
# add_drop_layer_norm
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_case(rows, E, p, seeded, affine=True, with_b=True):
    from e2ep_amd import _lib
    g = _g(rows * 3 + E if seeded else rows + E)
    leaves = {"a": torch.randn(rows, E, generator=g), "b": torch.randn(rows, E, generator=g)}
    u = torch.rand(rows, E, generator=g)
    if affine:
        leaves["gamma"] = 1 + 0.2 * torch.randn(E, generator=g)
        leaves["beta"] = 0.1 * torch.randn(E, generator=g)
    gy = torch.randn(rows, E, generator=g)
    if not with_b:
        del leaves["b"]
        consts, keep = {}, None
    elif seeded:  # the kernel's own keep mask, as test_add_dropout_layernorm_seeded takes it
        seed = torch.tensor([12345 + rows], dtype=torch.int32)
        kd = torch.empty(rows, E, dtype=torch.uint8, device=DEV)
        _lib.call("e2ep_attn_keep_mask", _lib.ptr(seed.to(DEV)), 1, rows, E, p, _lib.ptr(kd), _lib.stream())
        consts, keep = {"seed": seed}, kd.cpu().double()
    else:
        consts, keep = {"u": u}, (u >= p).double()

    def norm_of(t):
        norm = nn.LayerNorm(E, elementwise_affine=affine)
        if affine:
            norm.weight, norm.bias = t["gamma"], t["beta"]
        return norm

    def fn(t, c):
        from e2ep_amd import nn_ops
        return (nn_ops.add_drop_layer_norm(t["a"], t.get("b"), norm_of(t), p, u=c.get("u"),
                                           seed=c.get("seed")),), {}

    def ref(t, c):
        z = t["a"] + t["b"] * keep / (1 - p) if with_b else t["a"]
        return (norm_of(t)(z),), {}

    # test_nn_ops_gpu.py test_add_dropout_layernorm_fused / _seeded
    bounds = dict(y=1e-6, a=1e-5, b=1e-5, gamma=1e-5, beta=1e-5)
    return Case(("ln", rows, E, p, seeded, affine, with_b), leaves, consts, [gy], fn, ref, bounds)


LN_CASES = {"37x100_uniforms": (37, 100, 0.5, False), "7x33_seeded": (7, 33, 0.5, True)}
LN_SUBSETS = [("a",), ("b",), ("gamma", "beta"), ("a", "gamma")]


@pytest.mark.parametrize("shape", list(LN_CASES))
@pytest.mark.parametrize("subset", LN_SUBSETS, ids=_ids(LN_SUBSETS))
def test_add_drop_layer_norm(subset, shape):
    """The workspace for the column partials is taken only with dgamma or dbeta wanted; da / db
    are written under null checks; {a, gamma} leaves dbeta null in ln_param_grads_block."""
    check(ln_case(*LN_CASES[shape]), subset)


# ----------------------------------------------------------------------------------------------
# nn_ops.linear
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_case(rows, N, K, bias, relu, skip):
    g = _g(rows + N + K)
    leaves = {"x": torch.randn(rows, K, generator=g), "w": torch.randn(N, K, generator=g) * 0.1}
    if bias:
        leaves["b"] = torch.randn(N, generator=g)
    gys = [torch.randn(rows, N, generator=g)] + ([torch.randn(rows, K, generator=g)] if skip else [])

    def fn(t, c):
        from e2ep_amd import nn_ops
        out = nn_ops.linear(t["x"], t["w"], t.get("b"), skip=skip, relu=relu)
        return (out if skip else (out,)), {}

    def ref(t, c):
        y = F.linear(t["x"], t["w"], t.get("b"))
        y = y.clamp_min(0) if relu else y
        return ((y, t["x"] * 1) if skip else (y,)), {}

    bounds = dict(y0=2e-6, y1=2e-6, x=2e-6, w=2e-6, b=2e-6)  # test_gemm_gpu.py test_linear_autograd_vs_fp64
    return Case(("linear", rows, N, K, bias, relu, skip), leaves, {}, gys, fn, ref, bounds)


LINEAR_SHAPES = [(37, 70, 100), (112, 204, 258)]
# id -> (bias, relu, skip)
LINEAR_KINDS = {"bias": (True, False, False), "no_bias": (False, False, False),
                "relu": (True, True, False), "skip": (True, False, True)}
LINEAR_SUBSETS = [("x",), ("w",), ("b",), ("x", "w"), ("x", "b"), ("w", "b")]
LINEAR_PARAMS = [pytest.param(k, s, id=f"{k}-{'+'.join(s)}") for k in LINEAR_KINDS for s in LINEAR_SUBSETS
                 if LINEAR_KINDS[k][0] or "b" not in s]
# The all-gradients run is one k_gemm_pair launch (e2ep_linear_bwd).  A subset forks instead:
# dW with db is e2ep_gemm_rowsum and dX e2ep_gemm, both bitwise the pair's
# (test_linear_bwd_pair_bitwise_equals_two_launches).  The other two launch choices are not the
# pair's arithmetic.  w without b is e2ep_gemm, planned for an N x K output (gemm_plan(N, K,
# rows), or the skinny kernel) where the rowsum launch and the pair plan N x (K + 1) with the
# ones column: tile and K split, and so the order of each sum, may differ.  b without w is
# e2ep_col_sum, a column reduction of dY, where the pair's db is the ones column of the MFMA
# GEMM.  Those gradients keep (b); whether they happen to be equal is printed.
LINEAR_INEXACT = {("w",): ("w",), ("x", "w"): ("w",), ("b",): ("b",), ("x", "b"): ("b",)}


@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=["37x70x100", "112x204x258"])
@pytest.mark.parametrize("kind,subset", LINEAR_PARAMS)
def test_linear(kind, subset, shape):
    bias = LINEAR_KINDS[kind][0]
    # without a bias the all-gradients run is itself the fork with e2ep_gemm for dW
    inexact = LINEAR_INEXACT.get(subset, ()) if bias else ()
    check(linear_case(*shape, *LINEAR_KINDS[kind]), subset, inexact)


# ----------------------------------------------------------------------------------------------
# conv.conv2d, _Linear1x1
# ----------------------------------------------------------------------------------------------
# id -> (N, Cin, H, W, Cout, R, S, stride, pad, bias, grad_channels, skip)
CONVS = {"1x1_pair": (4, 24, 32, 32, 144, 1, 1, 1, (0, 0, 0, 0), True, None, False),
         "3x3": (2, 64, 16, 16, 64, 3, 3, 1, (1, 1, 1, 1), True, None, False),
         "3x3_s2": (2, 64, 16, 16, 128, 3, 3, 2, (1, 1, 1, 1), True, None, False),
         "3x3_nobias": (2, 64, 16, 16, 64, 3, 3, 1, (1, 1, 1, 1), False, None, False),
         "skip": (2, 64, 16, 16, 64, 3, 3, 1, (1, 1, 1, 1), False, None, True),
         "grad_channels": (2, 65, 16, 16, 64, 3, 3, 1, (1, 1, 1, 1), False, 64, True),
         "map_1x1": (8, 144, 1, 1, 6, 1, 1, 1, (0, 0, 0, 0), True, None, False)}


@functools.lru_cache(maxsize=None)
def conv_case(name, mode="fp32"):
    N, Cin, H, W, Cout, R, S, st, pad, bias, gc, skip = CONVS[name]
    g = _g(17 + Cin + Cout + R)
    leaves = {"x": torch.randn(N, Cin, H, W, generator=g),
              "w": torch.randn(Cout, Cin, R, S, generator=g) / (Cin * R * S) ** 0.5}
    if bias:
        leaves["b"] = torch.randn(Cout, generator=g)
    P, Q = (H + pad[2] + pad[3] - R) // st + 1, (W + pad[0] + pad[1] - S) // st + 1
    gys = [torch.randn(N, Cout, P, Q, generator=g)] + ([torch.randn(N, Cin, H, W, generator=g)] if skip else [])

    def fn(t, c):
        from e2ep_amd import conv
        out = conv.conv2d(t["x"], t["w"], t.get("b"), (st, st), pad, (1, 1), 0, grad_channels=gc, skip=skip)
        return (out if skip else (out,)), {}

    def ref(t, c):
        x = t["x"]
        if gc is not None:  # the channels past grad_channels get the skip gradient only
            x = torch.cat([x[:, :gc], x[:, gc:].detach()], 1)
        y = F.conv2d(F.pad(x, pad), t["w"], t.get("b"), st)
        return ((y, t["x"] * 1) if skip else (y,)), {}

    def precision_of():
        from e2ep_amd import precision
        return precision.use(mode)

    rnd = lambda v: v.bfloat16().float()  # noqa: E731
    if mode == "bf16":
        # operands rounded to bf16, fp32 products and sums: against fp64 of the rounded
        # operands (test_conv_gpu.py test_conv_low_precision_operands)
        assert not bias and not skip
        bounds = dict(y=2e-6, x=2e-6, w=5e-6)
        return Case(("conv", name, mode), leaves, {}, gys, fn, ref, bounds, (precision_of,),
                    {k: rnd(v) for k, v in leaves.items()}, [rnd(v) for v in gys])
    if skip:  # test_conv_gpu.py test_conv_skip_gradient_fused
        bounds = dict(y0=1e-5, y1=1e-5, x=1e-5, w=1e-5)
    else:     # test_conv_gpu.py test_conv_fwd_bwd_vs_fp64
        bounds = dict(y=2e-6, x=2e-6, w=2e-6, b=2e-6)
    return Case(("conv", name, mode), leaves, {}, gys, fn, ref, bounds)


CONV_SUBSETS = [("x",), ("w",), ("w", "b"), ("x", "b")]
MAP_SUBSETS = [("x",), ("w",), ("b",)]
BEV_SUBSETS = [("bev",), ("w",)]
GATE_SUBSETS = [("x",), ("a",)]


@pytest.mark.parametrize("layer", ["1x1_pair", "3x3", "3x3_s2"])
@pytest.mark.parametrize("subset", CONV_SUBSETS, ids=_ids(CONV_SUBSETS))
def test_conv2d(subset, layer):
    """All three layers pass e2ep_conv_bwd_pair_ok, so the all-gradients run is one
    k_conv_bwd_pair launch (+ e2ep_bias_grad) and a subset the data gradient, the weight
    gradient (forked only with x live) or the bias gradient alone: bitwise equal
    (test_conv_bwd_pair_bitwise_equals_two_launches)."""
    from e2ep_amd import _lib
    N, Cin, H, W, Cout, R, S, st, pad = CONVS[layer][:9]
    P, Q = (H + pad[2] + pad[3] - R) // st + 1, (W + pad[0] + pad[1] - S) // st + 1
    d = _lib.dims((N, Cin, H, W, Cout, R, S, P, Q, st, st, pad[2], pad[0], 1, 1))
    assert _lib.load().e2ep_conv_bwd_pair_ok(d, Cin) == 1
    check(conv_case(layer), subset)


@pytest.mark.parametrize("subset", XW_SUBSETS, ids=_ids(XW_SUBSETS))
def test_conv2d_bf16_operands(subset):
    check(conv_case("3x3_nobias", "bf16"), subset)


@pytest.mark.parametrize("layer", ["skip", "grad_channels"])
def test_conv2d_skip_with_frozen_weight(layer):
    """skip=True: the alias's gradient joins dx in the data-gradient epilogue; with w frozen
    that is the unpaired e2ep_conv_dgrad_acc with `res`.  grad_channels < Cin: the channels
    past it get the alias's gradient only."""
    check(conv_case(layer), ("x",))


@pytest.mark.parametrize("w_live", [True, False], ids=["w_live", "w_frozen"])
def test_conv2d_only_the_skip_alias_used(w_live):
    """conv2d(skip=True) whose y nobody reads: _Conv2d runs with set_materialize_grads(False),
    so its backward gets None for y.  y contributes nothing: x's gradient is the alias's, bit
    for bit, the weight gets none, and no kernel is launched on a None."""
    case = conv_case("skip")
    gs = case.gys[1]
    for fill in FILLS:
        with guard.allocations(fill) as g:
            from e2ep_amd import conv
            x = nn.Parameter(guard.put(case.leaves["x"]))
            w = nn.Parameter(guard.put(case.leaves["w"]), requires_grad=w_live)
            y, xs = conv.conv2d(x, w, None, (1, 1), (1, 1, 1, 1), (1, 1), 0, skip=True)
            xs.backward(guard.put(gs))
            torch.cuda.synchronize()
            assert torch.equal(x.grad.cpu(), gs) and w.grad is None
            assert rel_l2(y, _ref(case).ys[0]) < case.bounds["y0"]
            g.check()


def test_in_proj_qkv_refuses_an_unread_projection():
    """_InProjQKV also runs with set_materialize_grads(False) (for its two skip aliases).  A
    backward that reaches it with no gradient at q or at kv would leave that half of the one
    dW / db unwritten: it raises and names the op instead."""
    from e2ep_amd import _lib, nn_ops
    case = mha_case(True, 5, 9)
    x, mem, W, b = (nn.Parameter(case.leaves[k].to(DEV)) for k in ("x", "mem", "in_w", "in_b"))
    q, kv, qs, ks = nn_ops.in_proj_qkv(x, mem, W, b, E_ATT)
    with pytest.raises(_lib.E2EPError, match="in_proj_qkv"):
        q.sum().backward()
    assert W.grad is None and x.grad is None


@pytest.mark.parametrize("subset", MAP_SUBSETS, ids=_ids(MAP_SUBSETS))
def test_linear_1x1_map(subset):
    """_Linear1x1 (a 1x1 conv on a 1x1 map): three independent launches, one per gradient."""
    check(conv_case("map_1x1"), subset)


# ----------------------------------------------------------------------------------------------
# in_proj_qkv, attention.mha
# ----------------------------------------------------------------------------------------------
E_ATT, H_ATT, B_ATT = 258, 6, 2


@functools.lru_cache(maxsize=None)
def mha_case(cross, Sq, Sk):
    E = E_ATT
    g = _g(7 + Sq + Sk + cross)
    leaves = {"x": torch.randn(Sq, B_ATT, E, generator=g),
              "in_w": torch.randn(3 * E, E, generator=g) / E ** 0.5,
              "in_b": 0.1 * torch.randn(3 * E, generator=g),
              "out_w": torch.randn(E, E, generator=g) / E ** 0.5,
              "out_b": 0.1 * torch.randn(E, generator=g)}
    if cross:
        leaves["mem"] = torch.randn(Sk, B_ATT, E, generator=g)
    gy = torch.randn(Sq, B_ATT, E, generator=g)

    def module(t):
        m = nn.MultiheadAttention(E, H_ATT, dropout=0.0)
        m.in_proj_weight, m.in_proj_bias = t["in_w"], t["in_b"]
        m.out_proj.weight, m.out_proj.bias = t["out_w"], t["out_b"]
        return m

    def fn(t, c):
        from e2ep_amd import attention
        kv = t["mem"] if cross else t["x"]
        return (attention.mha(module(t), t["x"], kv, kv),), {}

    def ref(t, c):
        kv = t["mem"] if cross else t["x"]
        return (module(t)(t["x"], kv, kv, need_weights=False)[0],), {}

    bounds = {k: 1e-4 for k in list(leaves) + ["y"]}  # test_attention_gpu.py test_mha_matches_module
    return Case(("mha", cross, Sq, Sk), leaves, {}, [gy], fn, ref, bounds)


MHA_PARAMS = ("in_w", "in_b", "out_w", "out_b")


@pytest.mark.parametrize("Sq,Sk", [(5, 9), (14, 256)])
@pytest.mark.parametrize("kind", ["memory_detached", "module_frozen"])
def test_cross_attention(kind, Sq, Sk):
    """in_proj_qkv + attention + out_proj.  With every gradient wanted each half of the
    in-projection is one k_gemm_pair launch.  Memory detached: the kv half forks
    e2ep_gemm_rowsum into rows E.. of the one dW / db (bitwise the pair's,
    test_linear_bwd_pair_bitwise_equals_two_launches).  Module frozen: both halves and
    out_proj are e2ep_gemm data gradients alone."""
    need = ("x",) + MHA_PARAMS if kind == "memory_detached" else ("x", "mem")
    check(mha_case(True, Sq, Sk), need)


@pytest.mark.parametrize("S", [5, 14])
def test_self_attention_only_out_proj_trainable(S):
    """Nothing before out_proj is recorded by autograd; out_proj's backward is the
    e2ep_gemm_rowsum fork without a data gradient (bitwise the pair's dW / db)."""
    check(mha_case(False, S, S), ("out_w", "out_b"))


# ----------------------------------------------------------------------------------------------
# bev_stem, se_gate, cat_channels
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bev_stem_case():
    g = _g(77)
    leaves = {"bev": torch.randn(2, 64, 50, 50, generator=g)}
    consts = {"tgt": (torch.rand(2, 1, 50, 50, generator=g) > 0.9).float()}
    leaves["w"] = torch.randn(64, 65, 7, 7, generator=g) / (65 * 49) ** 0.5
    gy = torch.randn(2, 64, 32, 32, generator=g)

    def fn(t, c):
        from e2ep_amd import bev_stem
        return (bev_stem.bev_stem(t["bev"], c["tgt"], t["w"], (64, 64)),), {}

    def ref(t, c):
        x = F.interpolate(torch.cat([t["bev"], c["tgt"]], 1), size=(64, 64), mode="bilinear", align_corners=False)
        return (F.conv2d(x, t["w"], None, 2, 3),), {}

    bounds = dict(y=2e-5, bev=2e-5, w=2e-5)  # test_nn_ops_gpu.py test_bev_stem_resize_conv_fused
    return Case(("bev_stem",), leaves, consts, [gy], fn, ref, bounds)


@pytest.mark.parametrize("subset", BEV_SUBSETS, ids=_ids(BEV_SUBSETS))
def test_bev_stem(subset):
    """The weight gradient forks only with bev live; the data gradient and the channels-last
    resize backward run only for bev."""
    check(bev_stem_case(), subset)


@functools.lru_cache(maxsize=None)
def se_gate_case():
    g = _g(5)
    leaves = {"x": torch.randn(2, 16, 33, 64, generator=g), "a": torch.randn(2, 16, 1, 1, generator=g)}
    gy = torch.randn(2, 16, 33, 64, generator=g)

    def fn(t, c):
        from e2ep_amd import nn_ops
        return (nn_ops.se_gate(t["x"], t["a"]),), {}

    def ref(t, c):
        return (t["x"] * torch.sigmoid(t["a"]),), {}

    bounds = dict(y=1e-6, x=1e-6, a=1e-6)  # test_nn_ops_gpu.py test_maxpool_avgpool_segate
    return Case(("se_gate",), leaves, {}, [gy], fn, ref, bounds)


@pytest.mark.parametrize("subset", GATE_SUBSETS, ids=_ids(GATE_SUBSETS))
def test_se_gate(subset):
    """e2ep_se_gate_bwd writes both gradients; autograd drops the one not asked for."""
    check(se_gate_case(), subset)


@pytest.mark.parametrize("frozen", [0, 1, 2])
def test_cat_channels_one_piece_frozen(frozen):
    """e2ep_split_channels writes every piece; the frozen one's is dropped.  Pure data movement:
    each live piece's gradient is its slice of dy exactly (test_cat_channels_matches_torch)."""
    g = _g(3)
    chans = (1, 3, 2)
    leaves = {f"p{i}": torch.randn(2, c, 2, 2, generator=g) for i, c in enumerate(chans)}
    gy = torch.randn(2, sum(chans), 2, 2, generator=g)

    def fn(t, c):
        from e2ep_amd import nn_ops
        return (nn_ops.cat_channels([t[k] for k in sorted(t)]),), {}

    case = Case(("cat",), leaves, {}, [gy], fn, None, {})
    need = set(leaves) - {f"p{frozen}"}
    for fill in FILLS:
        r = _run(case, need, fill)
        assert torch.equal(r.ys[0], torch.cat([leaves[k] for k in sorted(leaves)], 1))
        c0 = 0
        for i, c in enumerate(chans):
            k = f"p{i}"
            assert (r.grads[k] is None) if i == frozen else torch.equal(r.grads[k], gy[:, c0:c0 + c]), k
            c0 += c


# ----------------------------------------------------------------------------------------------
# absent parameters: BatchNorm2d(affine=False), BatchNorm2d(track_running_stats=False),
# LayerNorm(elementwise_affine=False)
# ----------------------------------------------------------------------------------------------
# id -> (affine, track_running_stats, train).  A module without running statistics normalises
# with the batch's in eval too (torch.nn.BatchNorm2d.forward), so its eval case must equal the
# fp64 module's batch-statistics result.
ABSENT = {"no_affine_train": (False, True, True), "no_affine_eval": (False, True, False),
          "no_running_stats_train": (True, False, True), "no_running_stats_eval": (True, False, False),
          "neither_train": (False, False, True)}


@pytest.mark.parametrize("small", [1, 0], ids=["bn_one_launch", "bn_split"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=["3x7x5x9", "4x24x16x16"])
@pytest.mark.parametrize("kind", list(ABSENT))
def test_batch_norm_act_absent_parameters(kind, shape, small):
    affine, track, train = ABSENT[kind]
    check_full(bn_case(shape, small, "swish", True, False, train, affine, track))


@pytest.mark.parametrize("small", [1, 0], ids=["bn_one_launch", "bn_split"])
@pytest.mark.parametrize("dims", DW_DIMS, ids=DW_IDS)
@pytest.mark.parametrize("kind", list(ABSENT))
def test_bn_act_depthwise_conv2d_absent_parameters(kind, dims, small):
    affine, track, train = ABSENT[kind]
    check_full(dw_case(dims, True, small, train, affine, track))


@pytest.mark.parametrize("small", [1, 0], ids=["bn_one_launch", "bn_split"])
@pytest.mark.parametrize("shape", SE_SHAPES, ids=SE_IDS)
@pytest.mark.parametrize("kind", list(ABSENT))
def test_bn_swish_squeeze_excite_absent_parameters(kind, shape, small):
    affine, track, train = ABSENT[kind]
    check_full(se_case(shape, True, small, True, True, train, affine, track))


@pytest.mark.parametrize("kind", ["no_affine", "no_running_stats", "neither"])
def test_mbconv_mid_absent_parameters(kind):
    """e2ep_mbconv_mid_fwd / _bwd with null gamma / beta and null running buffers (what
    _bn_args hands through), against the fp64 modules built the same way and, bitwise, against
    the separate launches given the same nulls."""
    affine, track = kind == "no_running_stats", kind == "no_affine"
    case = mid_case(True, affine, track)
    runs = check_full(case)
    _mid_vs_separate(runs, set(case.leaves), affine, track)


@pytest.mark.parametrize("shape", list(LN_CASES))
def test_layer_norm_without_affine(shape):
    check_full(ln_case(*LN_CASES[shape], affine=False))


def test_add_drop_layer_norm_without_b():
    """e2ep.h: b of e2ep_add_drop_ln_fwd is nullable (y = norm(a)); the wrapper passes None on."""
    check_full(ln_case(37, 100, 0.0, False, with_b=False))


# ----------------------------------------------------------------------------------------------
# inside a deferral scope (defer.ParamGradDefer)
# ----------------------------------------------------------------------------------------------
DEFERRED = {"se-w2": (lambda: se_case(SE_SHAPES[1], False), ("w2",), True),
            "se-x": (lambda: se_case(SE_SHAPES[1], False), ("x",), False),
            "ln-gamma+beta": (lambda: ln_case(*LN_CASES["37x100_uniforms"]), ("gamma", "beta"), True),
            "ln-a": (lambda: ln_case(*LN_CASES["37x100_uniforms"]), ("a",), False),
            "conv-w": (lambda: conv_case("3x3"), ("w",), True)}


@pytest.mark.parametrize("name", list(DEFERRED))
def test_subset_inside_deferral_scope(name):
    """The SeRec / LnRec / SlabRec records carry the null output pointers to the batched
    launch of the flush.  Bitwise the immediate run; a case with a parameter gradient really
    defers (a record is pending before the flush), one without leaves nothing pending, and
    after the scope nothing is."""
    make, need, defers = DEFERRED[name]
    case = make()
    immediate = _run(case, set(need), guard.FILL_A)
    runs = check(case, need, scoped=True)
    for r in runs:
        assert (r.pending >= 1) if defers else (r.pending == 0), r.pending
        for k in need:
            assert torch.equal(r.grads[k], immediate.grads[k]), k

