"""Validation metrics, host side: the NumPy reference against the committed golden, the pure
host arithmetic of ValStep.finish, and the entry points' argument checks (no GPU is used: the
checks return before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import val_ref
from helpers import golden


def _labels():
    from e2ep_amd import synthetic
    d = synthetic.synthetic_batch(8, seed=11)
    return d["gt_acc"].numpy(), d["gt_steer"].numpy(), d["gt_reverse"].numpy()


def test_val_ref_reproduces_the_golden_validation_scalars():
    """val_ref (argmax of the logits, float64 after the detokenize) on the reference's own
    pred_control gives the reference's validation scalars.  The golden's scalars are fp32
    means of 32 fp32 terms: a few 2^-24 relative, held to 2e-6.  The golden's acc / steer rows
    are clear of the argmax-of-softmax ambiguity (smallest top-2 gap 5.8e-3)."""
    pc = golden("model_eval_b8.npz")["pred_control"]
    g = golden("validation_b8.npz")
    assert pc.shape == (8, 14, 204)
    assert val_ref.top2_gaps(pc).min() > 1e-3
    acc_steer, reverse = val_ref.control_val(pc, *_labels(), 204)
    assert abs(acc_steer / float(g["acc_steer_val_loss"]) - 1) < 2e-6
    assert abs(reverse / float(g["reverse_val_loss"]) - 1) < 2e-6
    # and the repository's torch ControlValLoss agrees on the CPU
    from loss.control_loss import ControlValLoss
    from tool.config import default_cfg
    a, s, r = _labels()
    data = {"gt_acc": torch.from_numpy(a), "gt_steer": torch.from_numpy(s),
            "gt_reverse": torch.from_numpy(r)}
    ta, tr = ControlValLoss(default_cfg())(torch.from_numpy(pc), data)
    assert abs(float(ta) / acc_steer - 1) < 2e-6 and abs(float(tr) / reverse - 1) < 2e-6


def test_val_ref_confusion_counts_and_ignores():
    x = np.zeros((1, 3, 2, 2), dtype=np.float32)
    x[0, 1, 0, 0] = 1.0          # pixel 0 -> class 1
    x[0, 2, 0, 1] = np.nan       # pixel 1 -> class 2 (NaN first)
    x[0, 0, 1, 0] = -np.inf      # pixel 2: tie of classes 1 and 2 -> 1
    t = np.array([[[1, 0], [2, 255]]])
    c = val_ref.confusion(x, t)
    assert c.tolist() == [[0, 0, 1], [0, 1, 0], [0, 1, 0]]
    assert val_ref.confusion(x, np.array([-1, 3, 255, 255])).sum() == 0


def _packed(rng, batches, C=3):
    from e2ep_amd.val import ValStep
    vals = rng.random((batches, 5))
    conf = rng.integers(0, 1000, (batches, C, C))
    sums = np.zeros(5)
    for v in vals:  # a running float64 sum, as the device keeps it
        sums = sums + v
    return ValStep.pack(sums, batches, conf.sum(0)), vals, conf


def test_finish_of_two_halves_equals_one_pass():
    from e2ep_amd.val import KEYS, ValStep
    rng = np.random.default_rng(5)
    whole, vals, conf = _packed(rng, 6)
    # the same batches accumulated by two ranks, then added as result() adds them
    halves = []
    for part_v, part_c in ((vals[:3], conf[:3]), (vals[3:], conf[3:])):
        s = np.zeros(5)
        for v in part_v:
            s = s + v
        halves.append(ValStep.unpack(ValStep.pack(s, len(part_v), part_c.sum(0))))
    merged = ValStep.pack(halves[0][0] + halves[1][0], halves[0][1] + halves[1][1],
                          halves[0][2] + halves[1][2])
    one, two = ValStep.finish(whole), ValStep.finish(merged)
    assert one["batches"] == two["batches"] == 6
    assert np.array_equal(one["seg_confusion"], two["seg_confusion"])
    assert np.array_equal(one["seg_confusion"], conf.sum(0))
    assert np.array_equal(one["seg_iou"], two["seg_iou"]) and one["seg_miou"] == two["seg_miou"]
    for i, k in enumerate(KEYS):
        # float64 sums of six values in [0, 1) regrouped: a few 2^-53 apart
        assert abs(one[k] - two[k]) < 1e-15
        assert abs(one[k] - vals[:, i].mean()) < 1e-15
    c = conf.sum(0)
    iou0 = c[0, 0] / (c[0].sum() + c[:, 0].sum() - c[0, 0])
    assert one["seg_iou"][0] == iou0
    assert abs(one["seg_miou"] - np.mean(one["seg_iou"])) < 1e-15


def test_iou_is_nan_on_an_absent_class_and_miou_skips_it():
    from e2ep_amd.val import ValStep
    conf = np.array([[5, 1, 0], [2, 4, 0], [0, 0, 0]])  # class 2 neither labelled nor predicted
    r = ValStep.finish(ValStep.pack([1.0, 2.0, 3.0, 4.0, 10.0], 2, conf))
    assert np.isnan(r["seg_iou"][2])
    assert r["seg_iou"][0] == 5 / 8 and r["seg_iou"][1] == 4 / 7
    assert r["seg_miou"] == (5 / 8 + 4 / 7) / 2
    assert r["val_loss"] == 5.0 and r["acc_steer_val_loss"] == 0.5 and r["batches"] == 2
    empty = ValStep.finish(ValStep.pack(np.zeros(5), 0, np.zeros((3, 3))))
    assert np.isnan(empty["val_loss"]) and np.isnan(empty["seg_miou"]) and empty["batches"] == 0
    plain = ValStep.finish(ValStep.pack(np.ones(5), 1))  # confusion=False
    assert "seg_iou" not in plain and plain["val_loss"] == 1.0
    from e2ep_amd import _lib
    with pytest.raises(_lib.E2EPError, match="packed"):
        ValStep.finish(np.zeros(48 + 8 * 5, dtype=np.uint8))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from e2ep_amd import _lib, losses
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    lib = _lib.load()
    EINVAL = _lib.CONSTANTS["E2EP_EINVAL"]
    buf = (ctypes.c_double * 64)()  # an aligned, non-null address; never dereferenced
    p = ctypes.c_void_p(ctypes.addressof(buf))
    ws = lambda B, F: lib.e2ep_control_val_workspace(B, F)  # noqa: E731

    def control(B, T, F, V=204, valid=200, split=101, pad=203, ptr=p, nbytes=None):
        return lib.e2ep_control_val_fwd(ptr, p, p, p, B, T, V, F, valid, split, pad, p, p,
                                        ws(B, F) if nbytes is None else nbytes, None)

    assert ws(8, 4) == 8 * 4 * 4 * 4
    assert control(1, 6, 1) == EINVAL            # (T - 2) % 3 != 0
    assert b"T=6" in lib.e2ep_last_error()
    assert control(1, 8, 1) == EINVAL            # F != (T - 2) / 3
    assert control(1, 2, 0) == EINVAL            # no control triple
    assert control(0, 5, 1) == EINVAL
    assert control(1, 5, 1, split=205) == EINVAL
    assert control(1, 5, 1, valid=0) == EINVAL
    assert control(1, 5, 1, ptr=None) == EINVAL
    assert control(1, 5, 1, nbytes=15) == EINVAL  # a short workspace

    def confusion(n, C, HW, nbytes=None):
        need = lib.e2ep_seg_confusion_workspace(n, HW)
        return lib.e2ep_seg_confusion(p, p, n, C, HW, 255, p, p, need if nbytes is None else nbytes,
                                      None)

    assert confusion(1, 9, 4) == EINVAL and b"C=9" in lib.e2ep_last_error()
    assert confusion(1, 1, 4) == EINVAL
    assert confusion(0, 3, 4) == EINVAL
    assert confusion(1, 3, 0) == EINVAL
    assert confusion(1, 3, 4, nbytes=8) == EINVAL
    assert lib.e2ep_val_accumulate(p, p, p, None, 3, p, p, None) == EINVAL  # C without a matrix
    assert lib.e2ep_val_accumulate(p, p, p, p, 9, p, p, None) == EINVAL
    assert lib.e2ep_val_accumulate(p, p, p, p, 3, None, p, None) == EINVAL
    # the Python wrappers: a CPU tensor raises, as for the training losses
    with pytest.raises(_lib.E2EPError, match="CPU tensor"):
        losses.control_val(torch.zeros(1, 5, 204), torch.zeros(1, 1), torch.zeros(1, 1),
                           torch.zeros(1, 1, dtype=torch.int64), 204)
    with pytest.raises(_lib.E2EPError, match="CPU tensor"):
        losses.seg_confusion(torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))
