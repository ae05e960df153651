"""NumPy statement of the reference's validation metrics (test infrastructure).

control_val: ControlValLoss.forward (reference loss/control_loss.py:45-75) with the argmax
taken on the fp32 logits, acc detokenised in Python doubles and rounded to fp32, steer in
fp32, everything after that in float64.  confusion: the segmentation confusion matrix by
np.bincount, the prediction being the first index of the largest logit with NaN first
(torch.argmax's order)."""
import numpy as np

SPLIT = 101


def argmax_first(x, axis):
    """torch.argmax's order along `axis`: first index of the largest value, a NaN above every
    number (np.argmax already treats NaN as the maximum and returns the first one)."""
    return np.argmax(x, axis=axis)


def smooth_l1(pred, gt):
    d = np.abs(pred.astype(np.float64) - gt.astype(np.float64))
    return np.where(d < 1.0, 0.5 * d * d, d - 0.5)


def top2_gaps(logits):
    """Per acc / steer row (k = 0, 1): largest minus second largest logit."""
    x = np.asarray(logits, dtype=np.float32)
    F = (x.shape[1] - 2) // 3
    rows = x[:, :3 * F].reshape(x.shape[0], F, 3, x.shape[2])[:, :, :2]
    s = np.sort(rows, axis=-1)
    return (s[..., -1] - s[..., -2]).reshape(-1)


def control_val(logits, gt_acc, gt_steer, gt_reverse, token_nums):
    """(acc_steer, reverse) as float64.  logits (B, 3 F + 2, V) fp32."""
    x = np.asarray(logits, dtype=np.float32)
    B, T, V = x.shape
    assert T >= 5 and (T - 2) % 3 == 0
    F = (T - 2) // 3
    ctrl = x[:, :T - 2]
    half = float((token_nums - 4) / 2)
    pad = token_nums - 1
    acc_tok = argmax_first(ctrl[:, 0::3], -1).reshape(-1)
    acc = np.array([(t / half - 1) if t > half else -(t / half - 1) for t in acc_tok.tolist()],
                   dtype=np.float32)
    acc_loss = smooth_l1(acc, np.asarray(gt_acc, dtype=np.float32).reshape(-1)).mean()
    steer_tok = argmax_first(ctrl[:, 1::3], -1).reshape(-1)
    steer = steer_tok.astype(np.float32) / np.float32(half) - np.float32(1)
    steer_loss = smooth_l1(steer, np.asarray(gt_steer, dtype=np.float32).reshape(-1)).mean()
    rev = ctrl[:, 2::3].astype(np.float64)
    e = np.exp(rev - rev.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    p_no, p_yes = p[..., :SPLIT].sum(-1).reshape(-1), p[..., SPLIT:].sum(-1).reshape(-1)
    t = np.asarray(gt_reverse).reshape(-1)
    keep = (t != pad) & ((t == 0) | (t == 1))
    lse = np.log(np.exp(p_no) + np.exp(p_yes))
    ce = lse - np.where(t == 0, p_no, p_yes)
    with np.errstate(invalid="ignore", divide="ignore"):
        rev_loss = ce[keep].sum() / np.float64(keep.sum())
    return float(acc_loss + steer_loss), float(rev_loss)


def confusion(logits, target, ignore=255):
    """(C, C) int64, rows = target class, columns = predicted class.  logits (n, C, ...)."""
    x = np.asarray(logits, dtype=np.float32)
    n, C = x.shape[:2]
    pred = argmax_first(x.reshape(n, C, -1), 1).reshape(-1)
    t = np.asarray(target).reshape(-1).astype(np.int64)
    keep = (t != ignore) & (t >= 0) & (t < C)
    return np.bincount(t[keep] * C + pred[keep], minlength=C * C).reshape(C, C).astype(np.int64)
