"""Depth-head metrics, host side: the NumPy reference (tests/depth_ref.py) against the labels
the reference's DepthLoss recorded (tests/golden/depth_cells.npz), the pure host arithmetic of
ValStep.finish_depth and pack_depth / unpack_depth, and the entry points' argument checks (no
GPU is used: the checks return before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import depth_ref
from helpers import golden


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_depth_ref_classes_equal_the_recorded_one_hot(name):
    g = golden("depth_cells.npz")
    d = g["depth_" + name]
    assert d.shape == (2, 3, 16, 24) and d.dtype == {"f32": np.float32, "f64": np.float64}[name]
    d_bound, down = g["d_bound"].tolist(), int(g["down"])
    assert d_bound == [0.5, 12.5, 0.25] and down == 8
    k, mn = depth_ref.classes(d.reshape(6, 16, 24), d_bound, down)
    onehot = g["onehot_" + name]
    assert onehot.shape == (36, 48)
    assert np.array_equal(np.eye(49, dtype=np.uint8)[k.reshape(-1)][:, 1:], onehot)
    k = k.reshape(2, 3, 2, 3)
    mn = mn.reshape(2, 3, 2, 3)
    # the planted cells: zeros, 0.25, 0.5, 12.49, 12.5, 1e5, a value among zeros, 0.75 - 1e-10
    assert mn[0, 0, 0, 0] == 1e5 and k[0, 0, 0, 0] == 0
    assert mn[0, 0, 0, 1] == 0.25 and k[0, 0, 0, 1] == 0
    assert mn[0, 1, 1, 0] == 0.5 and k[0, 1, 1, 0] == 1
    assert k[0, 2, 1, 2] == 48
    assert mn[1, 0, 0, 2] == 12.5 and k[1, 0, 0, 2] == 0
    assert mn[1, 1, 0, 0] == 1e5 and k[1, 1, 0, 0] == 0
    assert k[1, 2, 1, 1] == 1
    assert k[1, 2, 0, 0] == (2 if name == "f32" else 1)
    # the repository's torch statement of the same helper agrees
    from e2ep_amd import losses
    mine = losses.depth_onehot(torch.from_numpy(d), d_bound, down).numpy()
    assert np.array_equal(mine.astype(np.uint8), onehot)


def test_depth_ref_on_a_hand_worked_cell():
    """Two cameras, one cell each, D = 4, d_bound (1, 5, 1): z_d = 1 + d."""
    gt = np.array([[[2.5]], [[0.0]]], dtype=np.float32)  # camera 0: t = 1; camera 1: background
    prob = np.array([0.1, 0.2, 0.3, 0.4] * 2, dtype=np.float32).reshape(2, 4, 1, 1)
    r = depth_ref.depth_metrics(prob, gt, (1.0, 5.0, 1.0), 1, 2)
    assert r["cls"].reshape(-1).tolist() == [2, 0]
    assert r["counts"].tolist() == [[1, 0, 0, 2, 0], [0, 0, 0, 0, 0]]  # a = 3, 4 < 3.125 fails
    p = prob[0, :, 0, 0].astype(np.float64)
    ze = ((p[0] * 1.0 + p[1] * 2.0) + p[2] * 3.0) + p[3] * 4.0
    want = [1.5, 2.25, 0.6, abs(ze - 2.5), (ze - 2.5) ** 2, float(p[1])]
    assert r["sums"][0].tolist() == want and r["sums"][1].tolist() == [0.0] * 6
    assert r["pred_map"].reshape(-1).tolist() == [4.0, 4.0]
    assert r["gt_map"].reshape(-1).tolist() == [2.5, 0.0]
    # first NaN, then first largest
    rows = np.array([[1.0, 3.0, 3.0], [0.0, np.nan, np.nan]])
    assert depth_ref.argmax_first(rows).tolist() == [1, 1]


def test_finish_depth_arithmetic_and_an_empty_camera():
    from e2ep_amd.val import ValStep
    sums = np.array([[3.0, 8.0, 1.0, 2.0, 2.0, 1.0], [0.0] * 6, [1.0, 1.0, 0.5, 0.5, 0.25, 1.5]])
    counts = np.array([[4, 1, 2, 6, 3], [0] * 5, [2, 2, 2, 0, 2]])
    r = ValStep.finish_depth(ValStep.pack_depth(sums, counts, 7))
    pc = r["depth_per_camera"]
    assert set(pc) == set(r) - {"depth_per_camera"} and len(pc) == 11
    assert pc["depth_cells"].tolist() == [4, 0, 2] and r["depth_cells"] == 6
    assert pc["depth_bin_acc"][0] == 0.25 and pc["depth_bin_within1"][0] == 0.5
    assert pc["depth_bin_mae"][0] == 1.5 and pc["depth_delta125"][0] == 0.75
    assert pc["depth_abs_err"][0] == 0.75 and pc["depth_rmse"][0] == np.sqrt(2.0)
    assert pc["depth_abs_rel"][0] == 0.25 and pc["depth_exp_abs_err"][0] == 0.5
    assert pc["depth_exp_rmse"][0] == np.sqrt(0.5) and pc["depth_true_bin_prob"][0] == 0.25
    for k, v in pc.items():
        assert v.shape == (3,)
        assert k == "depth_cells" or (np.isnan(v[1]) and np.isfinite(v[[0, 2]]).all()), k
    assert pc["depth_bin_acc"][2] == 1.0 and pc["depth_true_bin_prob"][2] == 0.75
    assert r["depth_bin_acc"] == 3 / 6 and r["depth_bin_mae"] == 1.0
    assert r["depth_abs_err"] == 4.0 / 6 and r["depth_rmse"] == np.sqrt(9.0 / 6)
    assert r["depth_exp_rmse"] == np.sqrt(2.25 / 6) and r["depth_true_bin_prob"] == 2.5 / 6
    # no cell anywhere: every ratio NaN, also overall
    empty = ValStep.finish_depth(ValStep.pack_depth(np.zeros((2, 6)), np.zeros((2, 5)), 0))
    assert empty["depth_cells"] == 0 and np.isnan(empty["depth_rmse"])
    assert np.isnan(empty["depth_per_camera"]["depth_bin_acc"]).all()
    # one batch's `out` buffer (no batch counter behind it) is read the same way
    out_only = ValStep.pack_depth(sums, counts, 7)[:-8]
    assert ValStep.finish_depth(out_only)["depth_abs_err"] == r["depth_abs_err"]


def test_pack_depth_round_trip_and_wrong_sizes():
    from e2ep_amd import _lib, losses
    from e2ep_amd.val import ValStep
    rng = np.random.default_rng(3)
    for N in (1, 4, 16):
        sums = rng.random((N, 6)) * 1e3
        counts = rng.integers(0, 2 ** 50, (N, 5))
        raw = ValStep.pack_depth(sums, counts, 12345)
        assert raw.dtype == np.uint8 and raw.size == 88 * N + 8
        assert raw.size == losses.depth_metrics_bytes(N, running=True)
        assert losses.depth_metrics_bytes(N) == 88 * N
        s, c, b = ValStep.unpack_depth(raw)
        assert s.tobytes() == sums.tobytes() and np.array_equal(c, counts) and b == 12345
        s, c, b = ValStep.unpack_depth(raw[:-8])
        assert s.tobytes() == sums.tobytes() and np.array_equal(c, counts) and b is None
        # the device layout: sums[N][6] | counts[N][5] | batches
        assert raw[:48 * N].view(np.float64).tolist() == sums.reshape(-1).tolist()
        assert raw[48 * N:].view(np.int64).tolist() == counts.reshape(-1).tolist() + [12345]
    for size in (0, 8, 87, 88 + 4, 88 * 2 + 16):
        with pytest.raises(_lib.E2EPError, match="depth"):
            ValStep.unpack_depth(np.zeros(size, dtype=np.uint8))
        with pytest.raises(_lib.E2EPError, match="depth"):
            ValStep.finish_depth(np.zeros(size, dtype=np.uint8))
    with pytest.raises(_lib.E2EPError, match="depth"):
        ValStep.pack_depth(np.zeros((2, 5)), np.zeros((2, 5)), 0)
    with pytest.raises(_lib.E2EPError, match="depth"):
        ValStep.pack_depth(np.zeros((2, 6)), np.zeros((3, 5)), 0)


def test_depth_metrics_entry_points_refuse_bad_arguments_before_any_launch():
    from e2ep_amd import _lib, losses
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    lib = _lib.load()
    EINVAL = _lib.CONSTANTS["E2EP_EINVAL"]
    buf = (ctypes.c_double * 64)()  # an aligned, non-null address; never dereferenced
    p = ctypes.c_void_p(ctypes.addressof(buf))
    ws = lib.e2ep_depth_metrics_workspace
    assert ws(6, 3, 16, 24, 8) == 6 * 1 * 88          # one chunk per image
    assert ws(2, 1, 136, 136, 8) == 2 * 2 * 88        # 289 cells: two chunks
    assert ws(6, 4, 16, 24, 8) == 0 and ws(6, 0, 16, 24, 8) == 0 and ws(17, 17, 8, 8, 8) == 0
    assert ws(6, 3, 16, 20, 8) == 0 and ws(6, 3, 16, 24, 0) == 0

    for fn in (lib.e2ep_depth_metrics, lib.e2ep_depth_metrics_f64):
        def call(BN=6, N=3, D=48, H=16, W=24, down=8, prob=p, gt=p, out=p, work=p, nbytes=None):
            need = ws(6, 3, 16, 24, 8) if nbytes is None else nbytes
            return fn(prob, gt, BN, N, D, H, W, down, 0.25, 0.25, 0.5, 0.25, out, None, None, None,
                      None, work, need, None)

        assert call(N=0) == EINVAL and b"N=0" in lib.e2ep_last_error()
        assert call(BN=17, N=17) == EINVAL
        assert call(N=4) == EINVAL           # BN % N != 0
        assert call(BN=0) == EINVAL
        assert call(D=0) == EINVAL
        assert call(down=0) == EINVAL
        assert call(H=20) == EINVAL          # H % down != 0
        assert call(W=20) == EINVAL
        assert call(prob=None) == EINVAL and call(gt=None) == EINVAL
        assert call(out=None) == EINVAL and call(work=None) == EINVAL
        assert call(nbytes=6 * 88 - 1) == EINVAL and b"workspace" in lib.e2ep_last_error()
    # the Python wrapper: a CPU tensor raises, as for the losses
    with pytest.raises(_lib.E2EPError, match="CPU tensor"):
        losses.depth_metrics(torch.zeros(6, 48, 2, 3), torch.zeros(2, 3, 16, 24),
                             [0.5, 12.5, 0.25], 8, 3)
