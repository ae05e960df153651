"""The validation metric kernels (csrc/val.hip) on MI355X against tests/val_ref.py, every case
in guard-banded, poisoned buffers under both fills (tests/guard.py): the workspaces are taken
at exactly the queried size, so a store one element past them lands in a band.

Bounds.  control_val against the float64 reference: 1e-5 relative, the bound
test_model_b8_gpu holds the validation scalars to (the kernel's fp32 softmax, exp / log and
32-term fp32 means are a few 2^-24 each).  The confusion matrix and the accumulator are
integers and exactly rounded adds: equality."""
import numpy as np
import pytest
import torch

import guard
import val_ref
from helpers import golden

pytestmark = pytest.mark.gpu
FILLS = (guard.FILL_A, guard.FILL_B)
V = 204
TOKENS = (0, 100, 101, 199, 200, 203)  # both sides of half = 100, and the special tokens
DELTAS = (0.3, 1.7, -0.6, -2.2)        # |d| < 1 and |d| >= 1: both SmoothL1 branches


def _rel(a, b):
    return abs(float(a) / float(b) - 1)


def _control(pc, acc, steer, rev):
    """control_val under both fills; the two results must agree bit for bit."""
    from e2ep_amd import losses
    got = []
    for fill in FILLS:
        with guard.allocations(fill) as g:
            a, r = losses.control_val(guard.put(torch.from_numpy(pc)),
                                      guard.put(torch.from_numpy(acc)),
                                      guard.put(torch.from_numpy(steer)),
                                      guard.put(torch.from_numpy(rev)), V)
            assert guard.owns(a) and a.dtype == torch.float32 and a.dim() == 0 and r.dim() == 0
            got.append(torch.stack([a, r]).cpu().numpy())
            g.check()
    assert got[0].tobytes() == got[1].tobytes()
    return got[0]


def test_control_val_on_the_golden_logits():
    from e2ep_amd import synthetic
    pc = golden("model_eval_b8.npz")["pred_control"]
    g = golden("validation_b8.npz")
    d = synthetic.synthetic_batch(8, seed=11)
    got = _control(pc, d["gt_acc"].numpy(), d["gt_steer"].numpy(), d["gt_reverse"].numpy())
    e = (_rel(got[0], g["acc_steer_val_loss"]), _rel(got[1], g["reverse_val_loss"]))
    print("control_val vs golden:", got.tolist(), "rel", e)
    assert max(e) < 1e-5, (got, e)


def _detok_acc(t):
    return (t / 100.0 - 1) if t > 100.0 else -(t / 100.0 - 1)


def _planted(B, T, all_pad=False):
    """Seeded randn logits with +10 planted per row, so the argmax is known and far from the
    runner-up; labels that reach both SmoothL1 branches, both reverse classes, one pad and one
    label torch would assert on."""
    F = (T - 2) // 3
    rng = np.random.default_rng(100 * B + T)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    acc = np.zeros((B, F), dtype=np.float32)
    steer = np.zeros((B, F), dtype=np.float32)
    rev = np.zeros((B, F), dtype=np.int64)
    i = 0
    for b in range(B):
        for f in range(F):
            ta, ts, tr = TOKENS[i % 6], TOKENS[(i + 2) % 6], TOKENS[(i + 3) % 6]
            x[b, 3 * f, ta] += 10
            x[b, 3 * f + 1, ts] += 10
            x[b, 3 * f + 2, tr] += 10
            acc[b, f] = np.float32(_detok_acc(ta)) + np.float32(DELTAS[i % 4])
            steer[b, f] = np.float32(ts / 100.0 - 1) + np.float32(DELTAS[(i + 1) % 4])
            rev[b, f] = i % 2
            i += 1
    n = B * F
    if n >= 2:  # two exactly equal maxima in the last steer row: the first index wins
        x[B - 1, 3 * (F - 1) + 1, 150] = x[B - 1, 3 * (F - 1) + 1, 30] = 20.0
        rev[B - 1, F - 1] = V - 1  # pad: ignored
    if n >= 4:
        rev[0, 1] = 7  # neither 0 nor 1: ignored
    if all_pad:
        rev[:] = V - 1
    return x, acc, steer, rev


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [5, 14])
def test_control_val_on_planted_logits(B, T):
    x, acc, steer, rev = _planted(B, T)
    # argmax of the softmax is the reference's to define only where it cannot differ from the
    # argmax of the logits: the two largest logits equal, or clearly apart
    gaps = val_ref.top2_gaps(x)
    assert ((gaps == 0) | (gaps >= 1e-3)).all()
    if B * ((T - 2) // 3) >= 2:
        assert (gaps == 0).sum() == 1
    ref = val_ref.control_val(x, acc, steer, rev, V)
    got = _control(x, acc, steer, rev)
    e = (_rel(got[0], ref[0]), _rel(got[1], ref[1]))
    print(f"control_val B={B} T={T}:", got.tolist(), ref, "rel", e)
    assert max(e) < 1e-5, (got, ref, e)


def test_control_val_all_pad_reverse_is_nan():
    x, acc, steer, rev = _planted(3, 5, all_pad=True)
    ref = val_ref.control_val(x, acc, steer, rev, V)
    got = _control(x, acc, steer, rev)
    assert np.isnan(ref[1]) and np.isnan(got[1])
    assert _rel(got[0], ref[0]) < 1e-5


def test_control_val_refuses_a_row_count_that_is_not_3f_plus_2():
    from e2ep_amd import _lib, losses
    z = torch.zeros(1, 6, V, device="cuda")
    lab = torch.zeros(1, 1, device="cuda")
    with pytest.raises(_lib.E2EPError, match="T = 6"):
        losses.control_val(z, lab, lab, lab.long(), V)
    with pytest.raises(_lib.E2EPError, match="gt_steer"):
        losses.control_val(z[:, :5], lab, torch.zeros(1, 2, device="cuda"), lab.long(), V)


# ---- segmentation confusion matrix -------------------------------------------------------------
def _seg_case(n, C, X, Y):
    rng = np.random.default_rng(n * 1000 + C * 100 + X)
    x = (np.round(rng.standard_normal((n, C, X, Y)) * 2) / 2).astype(np.float32)  # exact ties
    t = rng.integers(0, C, (n, X, Y)).astype(np.int64)
    flat_x, flat_t = x.reshape(n, C, -1), t.reshape(-1)
    if X * Y >= 8:
        flat_x[0, 0, 0] = np.nan
        flat_x[0, C - 1, 1] = np.nan
        flat_x[0, 1, 1] = np.nan          # two NaNs in one pixel: the first wins
        flat_x[n - 1, C - 1, 2] = np.inf
        flat_x[n - 1, 0, 3] = -np.inf
        flat_x[n - 1, :, 4] = np.inf      # all equal at +inf
        flat_x[n - 1, :, X * Y - 1] = -np.inf
        flat_t[5] = 255
        flat_t[6] = -1
        flat_t[7] = C
        flat_t[-1] = 255
    return x, t


@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (1, 2, 1, 1), (2, 5, 16, 17), (2, 3, 200, 200)])
def test_seg_confusion_equals_bincount(shape):
    from e2ep_amd import losses
    x, t = _seg_case(*shape)
    ref = val_ref.confusion(x, t)
    assert ref.sum() == (t.size - (4 if t.size >= 8 else 0))
    for fill in FILLS:
        with guard.allocations(fill) as g:
            conf = losses.seg_confusion(guard.put(torch.from_numpy(x)), guard.put(torch.from_numpy(t)))
            assert guard.owns(conf) and conf.dtype == torch.int64
            # the same logits one element into a buffer: not 16-byte aligned, dword loads
            buf = guard.put(torch.from_numpy(np.concatenate([[0.0], x.reshape(-1)]).astype(np.float32)))
            off = buf[1:].view(shape)
            assert off.data_ptr() % 16 == 4 and off.is_contiguous()
            conf_off = losses.seg_confusion(off, guard.put(torch.from_numpy(t)))
            got, got_off = conf.cpu().numpy(), conf_off.cpu().numpy()
            g.check()
        assert np.array_equal(got, ref), (got, ref)
        assert np.array_equal(got_off, ref), (got_off, ref)


def test_seg_confusion_refuses_nine_classes():
    from e2ep_amd import _lib, losses
    with pytest.raises(_lib.E2EPError, match="classes"):
        losses.seg_confusion(torch.zeros(1, 9, 2, 2, device="cuda"),
                             torch.zeros(1, 2, 2, dtype=torch.int64, device="cuda"))
    with pytest.raises(_lib.E2EPError, match="target"):
        losses.seg_confusion(torch.zeros(1, 3, 2, 2, device="cuda"),
                             torch.zeros(1, 2, 3, dtype=torch.int64, device="cuda"))


# ---- epoch accumulator -----------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 0])
def test_val_accumulate_running_sums_are_exact(C):
    from e2ep_amd import _lib
    from e2ep_amd.val import ValStep
    rng = np.random.default_rng(9)
    vals = (rng.random((3, 4)) * 3).astype(np.float32)
    confs = rng.integers(0, 2 ** 40, (3, max(C, 1), max(C, 1))).astype(np.int64)
    for fill in FILLS:
        with guard.allocations(fill) as g:
            packed = torch.zeros(48 + 8 * C * C, dtype=torch.uint8, device="cuda")
            out = torch.empty((), dtype=torch.float32, device="cuda")
            sums, seen = np.zeros(5), []
            for v, c in zip(vals, confs):
                ctrl, seg = guard.put(torch.from_numpy(v[:2])), guard.put(torch.from_numpy(v[2:3]))
                depth = guard.put(torch.from_numpy(v[3:4]))
                conf = guard.put(torch.from_numpy(c)) if C else None
                _lib.call("e2ep_val_accumulate", _lib.ptr(ctrl), _lib.ptr(seg), _lib.ptr(depth),
                          _lib.ptr(conf), C, _lib.ptr(packed), _lib.ptr(out), _lib.stream())
                loss = np.float32(np.float32(np.float32(v[0] + v[1]) + v[2]) + v[3])
                seen.append(out.cpu().numpy().copy())
                assert seen[-1].tobytes() == loss.tobytes()
                sums = sums + np.concatenate([v.astype(np.float64), [np.float64(loss)]])
            host = packed.cpu().numpy()
            g.check()
        got_sums, batches, got_conf = ValStep.unpack(host)
        assert got_sums.tobytes() == sums.tobytes()  # float64 running sums, bit for bit
        assert batches == 3
        if C:
            assert np.array_equal(got_conf, confs.sum(0))
        else:
            assert got_conf is None
        r = ValStep.finish(host)
        assert r["val_loss"] == sums[4] / 3 and r["batches"] == 3
