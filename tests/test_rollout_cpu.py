"""The rollout metrics without a GPU: tests/rollout_ref.py (the statement the kernels are held to)
on hand-computed cases, its detokenisations against val_ref and the dataset's detokenize,
ValStep's host-only pack / unpack / finish for the third packed buffer, and the argument checks
that run before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import rollout_ref
import val_ref

V = 200                      # token_nums: valid_token 196, half 98
BOS, EOS, PAD = 197, 198, 199
KEYS = ("rollout_acc_l1", "rollout_steer_l1", "rollout_acc_token_acc", "rollout_steer_token_acc",
        "rollout_reverse_token_acc", "rollout_frame_exact", "rollout_prefix_exact",
        "rollout_reverse_acc", "rollout_invalid", "rollout_tf_agree_acc", "rollout_tf_agree_steer",
        "rollout_tf_agree_reverse")


def _seq(rows):
    return np.array([[BOS] + list(r) for r in rows], dtype=np.int64)


def _gtc(rows):
    return np.array([[BOS] + list(r) + [EOS, PAD] for r in rows], dtype=np.int64)


def test_detokenised_values_by_hand():
    toks = [98, 97, 99, 0, 196, PAD]
    s = rollout_ref.acc_signed(toks, V)
    v = rollout_ref.acc_folded(toks, V)
    st = rollout_ref.steer(toks, V)
    assert s.dtype == v.dtype == st.dtype == np.float32
    # half itself is not > half: the folded value takes the brake branch, -(0) = -0.0 == 0
    assert s[0] == 0.0 and v[0] == 0.0 and st[0] == 0.0
    assert s[1] == np.float32(97 / 98 - 1) and v[1] == np.float32(-(97 / 98 - 1)) and s[1] < 0 < v[1]
    assert s[2] == v[2] == np.float32(99 / 98 - 1) and s[2] > 0
    assert s[3] == -1.0 and v[3] == 1.0 and st[3] == -1.0
    assert s[4] == v[4] == st[4] == 1.0
    # an invalid id still detokenises: 199 / 98 - 1, beyond full throttle
    assert s[5] == v[5] == np.float32(199 / 98 - 1) and s[5] > 1
    assert st[5] == np.float32(199) / np.float32(98) - np.float32(1)


def test_signed_acceleration_is_detokenize_throttle_minus_brake():
    from dataset.carla_dataset import detokenize
    toks = np.arange(0, V - 4 + 1)
    got = rollout_ref.acc_signed(toks, V)
    for t in toks.tolist():
        throttle, brake, steer, _ = detokenize([t, t, 0], V)
        assert got[t] == np.float32(throttle - brake), t
        assert rollout_ref.acc_folded([t], V)[0] == np.float32(throttle + brake), t  # |.|
        assert abs(float(rollout_ref.steer([t], V)[0]) - steer) <= 2.0 ** -23, t


@pytest.mark.parametrize("tok", [0, 1, 97, 98, 99, 150, 196])
def test_folded_acc_and_steer_are_val_refs(tok):
    """One-hot teacher-forced logits make val_ref.control_val detokenise `tok`: its acc + steer
    scalar is the sum of this module's two SmoothL1 terms, bit for bit (F = 1: means of one)."""
    x = np.zeros((1, 5, V), dtype=np.float32)
    x[0, 0, tok] = x[0, 1, tok] = 5.0
    ga, gs = np.float32([[0.3]]), np.float32([[-1.7]])
    want = val_ref.control_val(x, ga, gs, np.zeros((1, 1), dtype=np.int64), V)[0]
    got = (val_ref.smooth_l1(rollout_ref.acc_folded([tok], V), ga.reshape(-1))[0]
           + val_ref.smooth_l1(rollout_ref.steer([tok], V), gs.reshape(-1))[0])
    assert float(got) == want


def test_statement_on_a_hand_computed_batch():
    """Three samples, three frames.  Sample 0 is right everywhere; sample 1 leaves the teacher's
    path at frame 1 (steer token) and is right again at frame 2: prefix_exact stays 0; sample 2
    decodes PAD at frame 0 and is wrong about reverse."""
    gt_rows = [[98, 97, 0, 99, 0, 196, 150, 98, 0]] * 3
    seq = _seq([gt_rows[0],
                [98, 97, 0, 99, 5, 196, 150, 98, 0],
                [PAD, 97, 196, 99, 0, 196, 150, 98, 196]])
    gtc = _gtc(gt_rows)
    ga = np.float32([[0.0, 0.5, 0.25]] * 3)
    gs = np.float32([[0.0, -1.0, 0.0]] * 3)
    gr = np.array([[0, 1, 0], [0, 1, 0], [0, 1, 7]], dtype=np.int64)
    # teacher-forced logits: the argmax is the ground truth everywhere but frame 2's acc row of
    # sample 1, where it is 3
    x = np.zeros((3, 11, V), dtype=np.float32)
    for b in range(3):
        for j, t in enumerate(gt_rows[b]):
            x[b, j, t] = 4.0
    x[1, 6, 3] = 9.0
    r = rollout_ref.rollout_metrics(seq, x, gtc, ga, gs, gr, V)
    c = r["counts"]
    assert c[:, 0].tolist() == [3, 3, 3]
    assert c[:, 1].tolist() == [2, 3, 3]          # acc token right
    assert c[:, 2].tolist() == [3, 2, 3]          # steer
    assert c[:, 3].tolist() == [2, 3, 2]          # reverse
    assert c[:, 4].tolist() == [2, 2, 2]          # frame exact
    assert c[:, 5].tolist() == [2, 1, 1]          # prefix: sample 1 never returns
    # reverse decision: frame 0 sample 2 says reverse against 0; frame 1 tokens 196 > 98 against
    # 1: right; frame 2 sample 2: the token says reverse and the label 7 is wrong whatever it says
    assert c[:, 6].tolist() == [2, 3, 2]
    assert c[:, 7].tolist() == [1, 0, 0]          # PAD decoded
    assert c[:, 8].tolist() == [2, 3, 2]          # agrees with the teacher-forced argmax
    assert c[:, 9].tolist() == [3, 2, 3]
    assert c[:, 10].tolist() == [2, 3, 2]
    s = r["sums"]
    pad_acc = float(np.float32(PAD / 98 - 1))
    assert s[0, 0] == 0.0 + 0.0 + pad_acc         # |acc_s - 0|
    assert s[0, 1] == 3 * abs(float(np.float32(97) / np.float32(98) - np.float32(1)))  # fp32
    assert s[0, 2] == (0.0 + 0.0) + (pad_acc - 0.5)   # SmoothL1's linear branch: d >= 1
    d = abs(float(np.float32(99 / 98 - 1)) - 0.5)
    assert s[1, 0] == (d + d) + d and s[1, 2] == (0.5 * d * d + 0.5 * d * d) + 0.5 * d * d
    e = abs(float(np.float32(5) / np.float32(98) - np.float32(1)) + 1.0)
    assert 0 < e < 1 and s[1, 1] == e and s[1, 3] == 0.5 * e * e   # token 0 is the label -1
    # without logits the agreement counts are 0 and nothing else moves
    r0 = rollout_ref.rollout_metrics(seq, None, gtc, ga, gs, gr, V)
    assert not r0["counts"][:, 8:].any()
    assert np.array_equal(r0["counts"][:, :8], c[:, :8])
    assert r0["sums"].tobytes() == s.tobytes()
    # a wider seq (the decode buffer's row) changes nothing
    wide = np.concatenate([seq, np.full((3, 4), PAD, dtype=np.int64)], 1)
    rw = rollout_ref.rollout_metrics(wide, x, gtc, ga, gs, gr, V)
    assert rw["sums"].tobytes() == s.tobytes() and np.array_equal(rw["counts"], c)


def test_pack_unpack_finish_rollout_round_trip():
    from e2ep_amd import _lib, losses
    from e2ep_amd.val import ValStep
    assert (losses.ROLLOUT_SUMS, losses.ROLLOUT_COUNTS) == (rollout_ref.SUMS, rollout_ref.COUNTS)
    rng = np.random.default_rng(5)
    for F in (1, 4, 7):
        sums = rng.random((F, 4)) * 1e3
        counts = rng.integers(0, 2 ** 50, (F, 11))
        raw = ValStep.pack_rollout(sums, counts, 321)
        assert raw.dtype == np.uint8 and raw.size == 120 * F + 8
        assert raw.size == losses.rollout_metrics_bytes(F, running=True)
        assert losses.rollout_metrics_bytes(F) == 120 * F
        s, c, b = ValStep.unpack_rollout(raw)
        assert s.tobytes() == sums.tobytes() and np.array_equal(c, counts) and b == 321
        s, c, b = ValStep.unpack_rollout(raw[:-8])
        assert s.tobytes() == sums.tobytes() and np.array_equal(c, counts) and b is None
        # the device layout: sums[F][4] | counts[F][11] | batches
        assert raw[:32 * F].view(np.float64).tolist() == sums.reshape(-1).tolist()
        assert raw[32 * F:].view(np.int64).tolist() == counts.reshape(-1).tolist() + [321]
    for size in (0, 8, 119, 120 + 4, 240 + 16):
        with pytest.raises(_lib.E2EPError, match="rollout"):
            ValStep.unpack_rollout(np.zeros(size, dtype=np.uint8))
        with pytest.raises(_lib.E2EPError, match="rollout"):
            ValStep.finish_rollout(np.zeros(size, dtype=np.uint8))
    with pytest.raises(_lib.E2EPError, match="rollout"):
        ValStep.pack_rollout(np.zeros((2, 3)), np.zeros((2, 11)), 0)
    with pytest.raises(_lib.E2EPError, match="rollout"):
        ValStep.pack_rollout(np.zeros((2, 4)), np.zeros((3, 11)), 0)


def test_finish_rollout_arithmetic_and_nan_at_zero_samples():
    from e2ep_amd.val import ValStep
    sums = np.array([[2.0, 1.0, 0.5, 0.25], [4.0, 3.0, 1.5, 0.75]])
    counts = np.array([[8, 4, 2, 8, 1, 1, 6, 0, 8, 4, 2], [8, 2, 2, 4, 0, 0, 8, 1, 4, 4, 8]])
    r = ValStep.finish_rollout(ValStep.pack_rollout(sums, counts, 2))
    assert set(r) == set(KEYS) | {"rollout_acc_steer_val_loss", "rollout_samples"}
    for k in KEYS:
        assert r[k].shape == (2,) and r[k].dtype == np.float64, k
    assert r["rollout_acc_l1"].tolist() == [0.25, 0.5]
    assert r["rollout_steer_l1"].tolist() == [0.125, 0.375]
    assert r["rollout_acc_token_acc"].tolist() == [0.5, 0.25]
    assert r["rollout_steer_token_acc"].tolist() == [0.25, 0.25]
    assert r["rollout_reverse_token_acc"].tolist() == [1.0, 0.5]
    assert r["rollout_frame_exact"].tolist() == [0.125, 0.0]
    assert r["rollout_prefix_exact"].tolist() == [0.125, 0.0]
    assert r["rollout_reverse_acc"].tolist() == [0.75, 1.0]
    assert r["rollout_invalid"].tolist() == [0.0, 0.125]
    assert r["rollout_tf_agree_acc"].tolist() == [1.0, 0.5]
    assert r["rollout_tf_agree_steer"].tolist() == [0.5, 0.5]
    assert r["rollout_tf_agree_reverse"].tolist() == [0.25, 1.0]
    assert r["rollout_acc_steer_val_loss"] == 2.0 / 16 + 1.0 / 16
    assert r["rollout_samples"] == 8
    # one batch's `out` buffer (no counter behind it) is read the same way
    assert ValStep.finish_rollout(ValStep.pack_rollout(sums, counts, 2)[:-8])[
        "rollout_acc_l1"].tolist() == [0.25, 0.5]
    empty = ValStep.finish_rollout(ValStep.pack_rollout(np.zeros((3, 4)), np.zeros((3, 11)), 0))
    assert empty["rollout_samples"] == 0 and np.isnan(empty["rollout_acc_steer_val_loss"])
    for k in KEYS:
        assert np.isnan(empty[k]).all() and empty[k].shape == (3,), k


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from e2ep_amd import _lib, losses
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    lib = _lib.load()
    EINVAL = _lib.CONSTANTS["E2EP_EINVAL"]
    buf = (ctypes.c_double * 64)()  # an aligned, non-null address; never dereferenced
    p = ctypes.c_void_p(ctypes.addressof(buf))
    ws = lib.e2ep_rollout_metrics_workspace
    assert ws(1, 1) == 3 * 24 and ws(16, 4) == 16 * 12 * 24
    assert ws(0, 4) == 0 and ws(2, 0) == 0 and ws(-1, -1) == 0

    def call(B=2, F=4, V=200, valid=196, stride=14, seq=p, gtc=p, acc=p, steer=p, rev=p, out=p,
             work=p, nbytes=None):
        need = ws(2, 4) if nbytes is None else nbytes
        return lib.e2ep_rollout_metrics(seq, stride, None, gtc, acc, steer, rev, B, F, V, valid,
                                        out, None, work, need, None)

    assert call(B=0) == EINVAL and b"B=0" in lib.e2ep_last_error()
    assert call(F=0) == EINVAL
    assert call(V=4) == EINVAL and b"vocab" in lib.e2ep_last_error()
    assert call(valid=0) == EINVAL
    assert call(stride=12) == EINVAL and b"stride" in lib.e2ep_last_error()
    assert call(nbytes=ws(2, 4) - 1) == EINVAL and b"workspace" in lib.e2ep_last_error()
    for name in ("seq", "gtc", "acc", "steer", "rev", "out", "work"):
        assert call(**{name: None}) == EINVAL, name
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    assert call(seq=odd) == EINVAL and b"misaligned" in lib.e2ep_last_error()
    # the Python wrapper: a CPU tensor raises, as for the losses
    z = torch.zeros(2, 4)
    with pytest.raises(_lib.E2EPError, match="CPU tensor"):
        losses.rollout_metrics(torch.zeros(2, 13, dtype=torch.int64), None,
                               torch.zeros(2, 15, dtype=torch.int64), z, z, z.long(), 200)
