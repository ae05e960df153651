"""NumPy statement of the depth-head metrics (include/e2ep.h, e2ep_depth_metrics), per camera:
the reference the kernel tests compare against.  The class map is DepthLoss's
(loss/depth_loss.py:32-48) evaluated in gt's own dtype, as torch evaluates it on such a tensor;
everything after it is float64 with one rounding per product and sum, in the kernel's order
within a cell (the expected depth adds its D terms with d ascending).  Across cells the sums
are math.fsum-exact here, so they bound what any summation order may give."""
import math

import numpy as np

SUMS, COUNTS = 6, 5


def cell_min(gt, down):
    """(BN, h, w) minimum of every down x down block of gt (BN, H, W), 0 read as 1e5, in gt's
    dtype."""
    BN, H, W = gt.shape
    g = gt.reshape(BN, H // down, down, W // down, down).transpose(0, 1, 3, 2, 4)
    g = g.reshape(BN, H // down, W // down, down * down)
    g = np.where(g == 0, gt.dtype.type(1e5), g)
    # a NaN depth never wins the kernel's `e < mn` (nor torch's min on these tests' inputs,
    # which hold no NaN)
    return np.where(np.isnan(g), gt.dtype.type(1e5), g).min(-1)


def classes(gt, d_bound, down, D=None):
    """(k int32 (BN, h, w), mn): DepthLoss's one-hot class (0 = background) and the cell
    minimum.  gt (BN, H, W) float32 or float64; the bin arithmetic runs in that dtype, with
    lo = d_bound[0] - d_bound[2] evaluated in Python floats first (loss/depth_loss.py:42)."""
    T = gt.dtype.type
    if D is None:
        D = int((d_bound[1] - d_bound[0]) / d_bound[2])
    mn = cell_min(gt, down)
    lo, step = T(d_bound[0] - d_bound[2]), T(d_bound[2])
    b = (mn - lo) / step
    assert b.dtype == gt.dtype
    ok = (b < T(D + 1)) & (b >= T(0))
    return np.where(ok, b, T(0)).astype(np.int64).astype(np.int32), mn


def argmax_first(p):
    """torch.argmax's order over the last axis: the first NaN, else the first largest."""
    nan = np.isnan(p)
    return np.where(nan.any(-1), nan.argmax(-1), np.where(nan, -np.inf, p).argmax(-1))


def depth_metrics(prob, gt, d_bound, down, n_cams):
    """prob (BN, D, h, w) float32, gt (BN, H, W) float32 / float64.  Returns a dict: sums
    (N, 6) float64, counts (N, 5) int64, pred_map and gt_map (BN, h, w) float32, cls int32."""
    BN, D, h, w = prob.shape
    d0, dstep = float(d_bound[0]), float(d_bound[2])
    k, mn = classes(gt, d_bound, down, D)
    fg = k >= 1
    t = k.astype(np.int64) - 1
    g = mn.astype(np.float64)
    p = np.moveaxis(prob, 1, -1)  # (BN, h, w, D)
    a = argmax_first(p).astype(np.int64)
    za = d0 + a.astype(np.float64) * dstep
    ze = np.zeros((BN, h, w))
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(D):
            ze = ze + p[..., d].astype(np.float64) * (d0 + float(d) * dstep)
    pt = np.take_along_axis(p, np.clip(t, 0, D - 1)[..., None], -1)[..., 0].astype(np.float64)
    db = np.abs(a - t)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        terms = [np.abs(za - g), (za - g) * (za - g), np.abs(za - g) / g, np.abs(ze - g),
                 (ze - g) * (ze - g), pt]
        flags = [fg, db == 0, db <= 1, db, (za < 1.25 * g) & (g < 1.25 * za)]
    sums, counts = np.zeros((n_cams, SUMS)), np.zeros((n_cams, COUNTS), dtype=np.int64)
    for n in range(n_cams):
        m = fg[n::n_cams]
        for e, v in enumerate(terms):
            sums[n, e] = math.fsum(v[n::n_cams][m].tolist()) if m.any() else 0.0
        for e, v in enumerate(flags):
            counts[n, e] = int(v[n::n_cams][m].astype(np.int64).sum())
    return {"sums": sums, "counts": counts, "pred_map": za.astype(np.float32),
            "gt_map": np.where(fg, mn, 0).astype(np.float32), "cls": k}
