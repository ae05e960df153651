"""The depth-metric kernels (csrc/val.hip, e2ep_depth_metrics / _f64) on MI355X against
tests/depth_ref.py.

Shapes: 6 cells per image (less than a wave) at D = 5 and D = 48, 45 cells (no multiple of 64),
25 cells at down = 1 (element loads of gt whatever the alignment), 289 cells (two workgroups
per image) and a single camera.  Every case plants, in image 0, the cells of
tests/golden/depth_cells.npz scaled to its d_bound (all zeros, a minimum of exactly lo, of
exactly d0, just under d1, exactly d1, all 1e5, one small value among zeros), a cell with two
equal largest probabilities, one with a NaN probability, one whose argmax is the last bin, an
exact hit and a miss by one bin (in the second sample's first image); with more than one camera the last camera sees only
background.

Bounds.  The ten counts, the class map and the two maps are integers or single roundings of
values the reference forms with the same operations: equality.  The six sums: every term is
bitwise NumPy's (float64, one rounding per operation, -ffp-contract=off) and non-negative, so
a sum of n <= 16 * 4096 terms in any order is within n * 2^-53 < 1e-11 relative of the exact
sum (math.fsum in depth_ref): held to 1e-9 relative."""
import functools

import numpy as np
import pytest
import torch

import depth_ref
import guard

pytestmark = pytest.mark.gpu
FILLS = (guard.FILL_A, guard.FILL_B)
BOUNDS = {48: (0.5, 12.5, 0.25), 5: (1.0, 6.0, 1.0)}
# (B, N, D, H, W, down)
SHAPES = [(2, 3, 5, 16, 24, 8), (2, 3, 48, 16, 24, 8), (2, 3, 48, 40, 72, 8), (2, 3, 5, 5, 5, 1),
          (2, 3, 48, 136, 136, 8), (2, 1, 48, 40, 72, 8)]
DTYPES = {"f32": np.float32, "f64": np.float64}
CASES = [(s, t) for s in SHAPES for t in DTYPES]
IDS = ["B{}N{}D{}_{}x{}d{}_{}".format(*s, t) for s, t in CASES]


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """(prob float32 (BN, D, h, w), gt (B, N, H, W) of dtype, d_bound, reference dict); built
    once and shared: nobody writes to it."""
    B, N, D, H, W, down = shape
    d0, d1, step = d_bound = BOUNDS[D]
    h, w = H // down, W // down
    rng = np.random.default_rng(hash(shape) % 2 ** 32)
    # a base depth per cell so that every bin (and both out-of-range sides) occurs, plus a
    # positive spread inside the cell and a sprinkle of zero (invalid) pixels
    base = rng.uniform(d0 - 2 * step, d1 + 2 * step, (B, N, h, 1, w, 1))
    gt = base + rng.uniform(0.0, 2.0, (B, N, h, down, w, down))
    gt = np.where(rng.random(gt.shape) < 0.1, 0.0, np.maximum(gt, 0.01))
    cells = gt.transpose(0, 1, 2, 4, 3, 5).reshape(B, N, h * w, down * down).copy()
    mid = d0 + 2.3 * step  # a foreground value: class 3

    def plant(i, fill, one=None):
        cells[0, 0, i] = fill
        if one is not None:
            cells[0, 0, i, (down * down) // 2] = one

    plant(0, 0.0)
    plant(1, d1 + 1.0, d0 - step)   # b = 0: background
    plant(2, d1 + 1.0, d0)          # b = 1: the first bin
    plant(3, d1 + 1.0, d1 - 0.01)   # the last bin
    plant(4, d1)                    # b = D + 1: out of range
    plant(5, 1e5)
    if down > 1:
        plant(0, 0.0, d0 + 0.8 * step)  # one small value among zeros
    TIE, NAN, LAST, HIT, NEAR = 0, 1, 2, 3, 4  # cells of image N: the second sample's camera 0
    for i in (TIE, NAN, LAST, HIT, NEAR):
        cells[1, 0, i] = mid
    if N > 1:
        cells[:, N - 1] = 0.0  # the last camera: no foreground cell in any image
    gt = cells.reshape(B, N, h, w, down, down).transpose(0, 1, 2, 4, 3, 5).reshape(B, N, H, W)
    gt = np.ascontiguousarray(gt).astype(DTYPES[dtype])
    k, _ = depth_ref.classes(gt.reshape(B * N, H, W), d_bound, down, D)
    # probabilities: a softmax pulled towards the true bin, at it or one or two bins off
    logits = rng.standard_normal((B * N, D, h, w)) * 2
    t = np.clip(k.astype(np.int64) - 1 + rng.integers(-2, 3, k.shape), 0, D - 1)
    np.put_along_axis(logits, t[:, None], np.take_along_axis(logits, t[:, None], 1) + 4, 1)
    e = np.exp(logits - logits.max(1, keepdims=True))
    prob = (e / e.sum(1, keepdims=True)).astype(np.float32).reshape(B * N, D, h * w)
    prob[N, :, TIE] = 0.01
    prob[N, 1, TIE] = prob[N, D - 2, TIE] = 0.45
    prob[N, 3, NAN] = np.nan
    prob[N, :, LAST] = 0.001
    prob[N, D - 1, LAST] = 0.99
    prob[N, :, HIT] = prob[N, :, NEAR] = 0.002
    prob[N, 2, HIT] = prob[N, 3, NEAR] = 0.9  # the true bin is 2: a hit and a miss by one
    prob = prob.reshape(B * N, D, h, w)
    ref = depth_ref.depth_metrics(prob, gt.reshape(B * N, H, W), d_bound, down, N)
    kk = ref["cls"].reshape(B, N, h * w)
    assert kk[0, 0, :6].tolist() == [1 if down > 1 else 0, 0, 1, D, 0, 0]
    assert kk[1, 0, [TIE, NAN, LAST]].tolist() == [3, 3, 3]
    a = depth_ref.argmax_first(np.moveaxis(prob, 1, -1)).reshape(B, N, h * w)
    assert a[1, 0, [TIE, NAN, LAST]].tolist() == [1, 3, D - 1]
    if N > 1:
        assert (ref["counts"][N - 1] == 0).all() and (ref["counts"][:N - 1, 0] > 0).all()
    assert (ref["counts"][0, :3] > 0).all()  # hits and near misses really occur
    assert np.isnan(ref["sums"][0, 3]) and np.isfinite(ref["sums"][:, :3]).all()
    return prob, gt, d_bound, ref


def _offset(x):
    """x one element into a guarded (or plain) buffer: not 16-byte aligned."""
    flat = torch.from_numpy(np.concatenate([np.zeros(1, x.dtype), x.reshape(-1)]))
    t = guard.put(flat)[1:].view(x.shape)
    assert t.data_ptr() % 16 == x.dtype.itemsize and t.is_contiguous()
    return t


def _run(prob, gt, d_bound, shape, running=None):
    """losses.depth_metrics with maps: (out bytes, pred_map, gt_map, cls) as host arrays."""
    from e2ep_amd import losses
    B, N, D, H, W, down = shape
    out, pm, gm, cls = losses.depth_metrics(prob, gt, d_bound, down, N, running=running, maps=True)
    assert out.dtype == torch.uint8 and out.numel() == 88 * N
    assert pm.dtype == gm.dtype == torch.float32 and cls.dtype == torch.int32
    return tuple(t.cpu().numpy() for t in (out, pm, gm, cls))


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _check(got, ref, what):
    from e2ep_amd.val import ValStep
    out, pm, gm, cls = got
    sums, counts, batches = ValStep.unpack_depth(out)
    assert batches is None
    print(what, "counts", counts.tolist())
    assert np.array_equal(counts, ref["counts"]), (what, counts, ref["counts"])
    assert np.array_equal(cls, ref["cls"]), what
    assert pm.tobytes() == ref["pred_map"].tobytes(), what
    assert gm.tobytes() == ref["gt_map"].tobytes(), what
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(sums - ref["sums"]) / np.abs(ref["sums"])
    rel = np.where(sums == ref["sums"], 0.0, rel)
    print(what, "largest relative error of a sum", np.nanmax(rel))
    assert np.array_equal(np.isnan(sums), np.isnan(ref["sums"])), (what, sums, ref["sums"])
    assert (rel[~np.isnan(ref["sums"])] < 1e-9).all(), (what, sums, ref["sums"])


@pytest.mark.parametrize("shape, dtype", CASES, ids=IDS)
def test_depth_metrics_equal_the_reference(shape, dtype):
    """Aligned and offset operands, unguarded and in guard-banded buffers under both fills:
    all against depth_ref, and all the same bits."""
    prob, gt, d_bound, ref = _case(shape, dtype)
    plain = _run(guard.put(torch.from_numpy(prob)), guard.put(torch.from_numpy(gt)), d_bound, shape)
    _check(plain, ref, "plain")
    again = _run(guard.put(torch.from_numpy(prob)), guard.put(torch.from_numpy(gt)), d_bound, shape)
    assert _same(plain, again)  # two runs, the same bits
    off = _run(_offset(prob), _offset(gt), d_bound, shape)
    _check(off, ref, "offset")
    assert _same(plain, off)  # element loads visit the same cells in the same order
    for fill in FILLS:
        with guard.allocations(fill) as g:
            p, t = guard.put(torch.from_numpy(prob)), guard.put(torch.from_numpy(gt))
            assert guard.owns(p) and p.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0
            got = _run(p, t, d_bound, shape)
            got_off = _run(_offset(prob), _offset(gt), d_bound, shape)
            g.check()
        assert _same(plain, got) and _same(plain, got_off), hex(fill)


@pytest.mark.parametrize("shape, dtype", CASES, ids=IDS)
def test_cls_out_is_the_depth_loss_class_map(shape, dtype):
    """cls_out against the cls a direct e2ep_depth_bce_fwd / _f64 call writes on the same
    tensors."""
    from e2ep_amd import _lib
    B, N, D, H, W, down = shape
    prob, gt, d_bound, ref = _case(shape, dtype)
    p, t = torch.from_numpy(prob).cuda(), torch.from_numpy(gt).cuda()
    got = _run(p, t, d_bound, shape)[3]
    h, w = H // down, W // down
    loss, den = torch.empty((), device="cuda"), torch.empty(1, device="cuda")
    cls = torch.full((B * N * h * w,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(_lib.call_raw("e2ep_depth_bce_workspace", B * N, H, W, down), 16),
                     dtype=torch.uint8, device="cuda")
    fn = "e2ep_depth_bce_fwd_f64" if dtype == "f64" else "e2ep_depth_bce_fwd"
    _lib.call(fn, _lib.ptr(p), _lib.ptr(t), B * N, D, H, W, down, d_bound[0] - d_bound[2],
              d_bound[2], _lib.ptr(loss), _lib.ptr(den), _lib.ptr(cls), _lib.ptr(ws), _lib.stream())
    assert np.array_equal(cls.cpu().numpy(), got.reshape(-1))
    assert np.array_equal(got, ref["cls"])


@pytest.mark.parametrize("shape, dtype", [CASES[2], CASES[9], CASES[11]],
                         ids=[IDS[2], IDS[9], IDS[11]])
def test_running_is_the_sequential_sum_of_three_calls(shape, dtype):
    from e2ep_amd import losses
    from e2ep_amd.val import ValStep
    B, N, D, H, W, down = shape
    prob, gt, d_bound, _ = _case(shape, dtype)
    t = torch.from_numpy(gt).cuda()
    for fill in FILLS:
        with guard.allocations(fill) as g:
            running = torch.zeros(losses.depth_metrics_bytes(N, running=True), dtype=torch.uint8,
                                  device="cuda")
            outs = []
            for i in range(3):  # three different batches: the bins rolled
                p = guard.put(torch.from_numpy(np.roll(prob, i, axis=1)))
                out = losses.depth_metrics(p, t, d_bound, down, N, running=running)
                outs.append(ValStep.unpack_depth(out.cpu().numpy()))
            host = running.cpu().numpy()
            g.check()
        sums, counts, batches = ValStep.unpack_depth(host)
        want_s, want_c = np.zeros((N, 6)), np.zeros((N, 5), dtype=np.int64)
        for s, c, _ in outs:
            want_s, want_c = want_s + s, want_c + c
        assert batches == 3
        assert sums.tobytes() == want_s.tobytes() and np.array_equal(counts, want_c)
        assert not np.array_equal(outs[0][1], outs[1][1])  # the batches really differ
        r = ValStep.finish_depth(host)
        assert r["depth_cells"] == int(want_c[:, 0].sum())
        if N > 1:
            assert np.isnan(r["depth_per_camera"]["depth_bin_acc"][N - 1])


def test_bad_arguments_return_einval_and_the_wrapper_raises():
    from e2ep_amd import _lib, losses
    lib = _lib.load()
    EINVAL = _lib.CONSTANTS["E2EP_EINVAL"]
    prob = torch.full((6, 5, 2, 3), 0.2, device="cuda")
    gt = torch.ones(2, 3, 16, 24, device="cuda")
    out = torch.zeros(88 * 3, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(lib.e2ep_depth_metrics_workspace(6, 3, 16, 24, 8), dtype=torch.uint8,
                     device="cuda")

    def call(BN=6, N=3, D=5, H=16, W=24, down=8, gt_=gt, nbytes=ws.numel(), out_=out):
        return lib.e2ep_depth_metrics(_lib.ptr(prob), _lib.ptr(gt_), BN, N, D, H, W, down, 0.0, 1.0,
                                      1.0, 1.0, _lib.ptr(out_), None, None, None, None,
                                      _lib.ptr(ws), nbytes, _lib.stream())

    assert call() == 0
    for bad in (dict(N=0), dict(N=4), dict(BN=34, N=17), dict(D=0), dict(down=0), dict(H=20),
                dict(W=20), dict(gt_=None), dict(out_=None), dict(nbytes=ws.numel() - 1)):
        assert call(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    with pytest.raises(_lib.E2EPError, match="cameras"):
        losses.depth_metrics(prob, gt, BOUNDS[5], 8, 4)
    with pytest.raises(_lib.E2EPError, match="prob"):
        losses.depth_metrics(prob[:, :4], gt, BOUNDS[5], 8, 3)
    with pytest.raises(_lib.E2EPError, match="running"):
        losses.depth_metrics(prob, gt, BOUNDS[5], 8, 3, running=out)
