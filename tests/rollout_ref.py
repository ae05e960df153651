"""NumPy statement of the free-running rollout metrics (csrc/val.hip, e2ep_rollout_metrics;
test infrastructure).

Per sample b, future frame f and k = 0, 1, 2 (acc, steer, reverse): p = seq[b][1 + 3f + k] is
the decoder's own token, g = gt_control[b][1 + 3f + k] the ground truth's, a the argmax of the
teacher-forced logits[b][3f + k] in torch.argmax's order (val_ref.argmax_first).  SmoothL1 is
val_ref.smooth_l1 (float64 from the two fp32 values).  val_ref states the two detokenisations
inline in control_val, so acc_folded and steer below repeat those two expressions word for word
and test_rollout_cpu.py holds them to val_ref.control_val on one-hot logits.  Every sum adds
its terms over b in index order in float64; the counts are integers."""
import numpy as np

import val_ref

SUMS, COUNTS = 4, 11


def half(token_nums):
    return float((token_nums - 4) / 2)


def acc_signed(tok, token_nums):
    """The acceleration the agent executes, throttle - brake of detokenize: token / half - 1 in
    Python doubles, rounded to fp32."""
    h = half(token_nums)
    return np.array([t / h - 1 for t in np.asarray(tok).reshape(-1).tolist()], dtype=np.float32)


def acc_folded(tok, token_nums):
    """ControlValLoss.detokenize_acc as val_ref.control_val runs it: folded at half."""
    h = half(token_nums)
    return np.array([(t / h - 1) if t > h else -(t / h - 1)
                     for t in np.asarray(tok).reshape(-1).tolist()], dtype=np.float32)


def steer(tok, token_nums):
    """ControlValLoss.detokenize_steer as val_ref.control_val runs it: fp32 arithmetic."""
    t = np.asarray(tok).reshape(-1)
    return t.astype(np.float32) / np.float32(half(token_nums)) - np.float32(1)


def rollout_metrics(seq, logits, gt_control, gt_acc, gt_steer, gt_reverse, token_nums):
    """{'sums': float64 (F, 4), 'counts': int64 (F, 11)} in the entry point's order.  seq
    (B, >= 1 + 3 F) int64, logits (B, 3 F + 2, V) fp32 or None, gt_control (B, 3 F + 3)."""
    seq, gtc = np.asarray(seq, dtype=np.int64), np.asarray(gt_control, dtype=np.int64)
    ga = np.asarray(gt_acc, dtype=np.float32)
    gs = np.asarray(gt_steer, dtype=np.float32)
    gr = np.asarray(gt_reverse, dtype=np.int64)
    B, F = ga.shape
    assert seq.shape[0] == B and seq.shape[1] >= 1 + 3 * F and gtc.shape == (B, 3 * F + 3)
    valid = token_nums - 4
    h = half(token_nums)
    p = seq[:, 1:1 + 3 * F].reshape(B, F, 3)
    g = gtc[:, 1:1 + 3 * F].reshape(B, F, 3)
    hit = p == g
    if logits is None:
        agree = np.zeros((B, F, 3), dtype=bool)
    else:
        x = np.asarray(logits, dtype=np.float32)
        assert x.shape[:2] == (B, 3 * F + 2)
        agree = p == val_ref.argmax_first(x[:, :3 * F], -1).reshape(B, F, 3)
    invalid = p > valid
    sums = np.zeros((F, SUMS), dtype=np.float64)
    counts = np.zeros((F, COUNTS), dtype=np.int64)
    for f in range(F):
        a_s = acc_signed(p[:, f, 0], token_nums)
        a_v = acc_folded(p[:, f, 0], token_nums)
        st = steer(p[:, f, 1], token_nums)
        terms = (np.abs(a_s.astype(np.float64) - ga[:, f].astype(np.float64)),
                 np.abs(st.astype(np.float64) - gs[:, f].astype(np.float64)),
                 val_ref.smooth_l1(a_v, ga[:, f]), val_ref.smooth_l1(st, gs[:, f]))
        for e, t in enumerate(terms):
            s = np.float64(0.0)
            for b in range(B):
                s = s + t[b]
            sums[f, e] = s
        rev = p[:, f, 2].astype(np.float64) > h
        right = np.where(gr[:, f] == 1, rev, np.where(gr[:, f] == 0, ~rev, False))
        counts[f] = (B, hit[:, f, 0].sum(), hit[:, f, 1].sum(), hit[:, f, 2].sum(),
                     hit[:, f].all(-1).sum(), hit[:, :f + 1].all((1, 2)).sum(), right.sum(),
                     invalid[:, f].any(-1).sum(), agree[:, f, 0].sum(), agree[:, f, 1].sum(),
                     agree[:, f, 2].sum())
    return {"sums": sums, "counts": counts}
