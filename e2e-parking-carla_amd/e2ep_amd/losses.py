"""The three training losses (reference loss/*.py) as autograd ops over the fused HIP loss
kernels (csrc/loss.hip): two launches forward (rows/blocks -> one fixed-order final sum),
one backward, no host synchronisation, no PyTorch arithmetic.  The nn.Module wrappers in
loss/ keep the reference's classes and signatures.  control_val, seg_confusion, depth_metrics
and rollout_metrics are the validation metrics (csrc/val.hip): forward only, two launches
each."""
import torch

from . import _lib


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.E2EPError("e2ep losses run on a HIP device only; got a CPU tensor")


def _i64(t, device):
    return t.to(device=device, dtype=torch.int64, non_blocking=True).contiguous()


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


class _ControlCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, pad):
        pred = pred.contiguous()
        B, T, V = pred.shape
        f32 = dict(dtype=torch.float32, device=pred.device)
        loss, lse, count = torch.empty((), **f32), torch.empty(B * T, **f32), torch.empty(1, **f32)
        ws = _ws(_lib.load().e2ep_control_ce_workspace(B * T), pred.device)
        _lib.call("e2ep_control_ce_fwd", _lib.ptr(pred), _lib.ptr(gt), B, T, gt.shape[1], 1, V, pad,
                  _lib.ptr(loss), _lib.ptr(lse), _lib.ptr(count), _lib.ptr(ws), _lib.stream())
        ctx.save_for_backward(pred, gt, lse, count)
        ctx.pad = pad
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, gt, lse, count = ctx.saved_tensors
        B, T, V = pred.shape
        d = torch.empty_like(pred)
        _lib.call("e2ep_control_ce_bwd", _lib.ptr(pred), _lib.ptr(gt), _lib.ptr(lse), _lib.ptr(count),
                  _lib.ptr(g.contiguous()), B, T, gt.shape[1], 1, V, ctx.pad, _lib.ptr(d), _lib.stream())
        return d, None, None


def control_ce(pred, gt_control, pad_idx):
    """loss/control_loss.py:15-19: CE over (B*T, vocab) logits vs gt[:, 1:], PAD ignored.
    pred (B, T, vocab) fp32, gt_control (B, T+1) token ids."""
    _dev(pred)
    gt = _i64(gt_control, pred.device)
    if pred.dim() != 3 or gt.shape[1] != pred.shape[1] + 1 or gt.shape[0] != pred.shape[0]:
        raise _lib.E2EPError(f"control_ce: pred {tuple(pred.shape)} vs gt_control {tuple(gt.shape)}")
    return _ControlCE.apply(pred, gt, int(pad_idx))


class _SegCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weights, ignore):
        pred = pred.contiguous()
        n, C = pred.shape[0], pred.shape[1]
        HW = pred[0, 0].numel()
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        ws = _ws(_lib.load().e2ep_seg_ce_workspace(n, HW), pred.device)
        _lib.call("e2ep_seg_ce_fwd", _lib.ptr(pred), _lib.ptr(target), _lib.ptr(weights), n, C, HW,
                  ignore, _lib.ptr(loss), _lib.ptr(ws), _lib.stream())
        ctx.save_for_backward(pred, target, weights)
        ctx.ignore = ignore
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, target, weights = ctx.saved_tensors
        n, C = pred.shape[0], pred.shape[1]
        HW = pred[0, 0].numel()
        d = torch.empty_like(pred)
        _lib.call("e2ep_seg_ce_bwd", _lib.ptr(pred), _lib.ptr(target), _lib.ptr(weights),
                  _lib.ptr(g.contiguous()), n, C, HW, ctx.ignore, _lib.ptr(d), _lib.stream())
        return d, None, None, None


def seg_weighted_ce(pred, target, weights, ignore_index=255):
    """loss/seg_loss.py:12-26: per-pixel weighted CE, then a plain mean over pixels.
    pred (b, s, C, H, W) logits, target (b, s, H, W) class ids, weights (C,)."""
    _dev(pred)
    b, s, c, h, w = pred.shape
    tg = _i64(target, pred.device).view(b * s, h * w)
    wt = weights.to(device=pred.device, dtype=torch.float32).contiguous()
    return _SegCE.apply(pred.reshape(b * s, c, h, w), tg, wt, int(ignore_index))


REVERSE_SPLIT = 101  # loss/control_loss.py:69-70: the reverse mass is split at token 101


def control_val_out(pred, gt_acc, gt_steer, gt_reverse, token_nums):
    """control_val's two scalars as one (2,) fp32 tensor (acc_steer, reverse)."""
    _dev(pred)
    if pred.dim() != 3 or pred.dtype != torch.float32:
        raise _lib.E2EPError(f"control_val: pred must be (B, T, vocab) fp32, got {pred.dtype} "
                             f"{tuple(pred.shape)}")
    B, T, V = pred.shape
    if T < 5 or (T - 2) % 3 != 0:
        raise _lib.E2EPError(f"control_val: pred has T = {T} rows per sample, expected 3 F + 2 "
                             "(F control triples, EOS, PAD)")
    F = (T - 2) // 3
    for name, t in (("gt_acc", gt_acc), ("gt_steer", gt_steer), ("gt_reverse", gt_reverse)):
        if tuple(t.shape) != (B, F):
            raise _lib.E2EPError(f"control_val: {name} {tuple(t.shape)} vs pred {tuple(pred.shape)}"
                                 f" (expected {(B, F)})")
    token_nums = int(token_nums)
    if token_nums <= 4:
        raise _lib.E2EPError(f"control_val: token_nums {token_nums} leaves no control tokens")
    dev = pred.device
    with torch.no_grad():
        pred = pred.detach().contiguous()
        acc = gt_acc.detach().to(device=dev, dtype=torch.float32).contiguous()
        steer = gt_steer.detach().to(device=dev, dtype=torch.float32).contiguous()
        rev = _i64(gt_reverse.detach(), dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.call_raw("e2ep_control_val_workspace", B, F), dtype=torch.uint8,
                         device=dev)
        _lib.call("e2ep_control_val_fwd", _lib.ptr(pred), _lib.ptr(acc), _lib.ptr(steer),
                  _lib.ptr(rev), B, T, V, F, token_nums - 4, min(REVERSE_SPLIT, V), token_nums - 1,
                  _lib.ptr(out), _lib.ptr(ws), _lib.nbytes(ws), _lib.stream())
    return out


def control_val(pred, gt_acc, gt_steer, gt_reverse, token_nums):
    """loss/control_loss.py:45-75 (ControlValLoss.forward) in two launches: (acc_steer_val_loss,
    reverse_val_loss) as device scalars.  pred (B, 3 F + 2, token_nums) fp32 logits, gt_acc and
    gt_steer (B, F), gt_reverse (B, F) token ids.  No autograd: these are metrics.  The tokens
    are the argmax of the logits (the reference's argmax of the fp32 softmax, except where two
    distinct logits round to equal probabilities: csrc/val.hip)."""
    out = control_val_out(pred, gt_acc, gt_steer, gt_reverse, token_nums)
    return out[0], out[1]


def seg_confusion(pred, target, ignore_index=255):
    """The (C, C) int64 confusion matrix of segmentation logits against their labels, rows =
    target class, columns = predicted class (the per-pixel argmax the agent steers by, in
    torch.argmax's order).  pred (n, C, X, Y) fp32 logits, target n * X * Y class ids in any
    shape; a pixel whose label is ignore_index or outside [0, C) is counted nowhere."""
    _dev(pred)
    if pred.dim() != 4 or pred.dtype != torch.float32:
        raise _lib.E2EPError(f"seg_confusion: pred must be (n, C, X, Y) fp32, got {pred.dtype} "
                             f"{tuple(pred.shape)}")
    n, C, X, Y = pred.shape
    if not 2 <= C <= 8:
        raise _lib.E2EPError(f"seg_confusion: {C} classes, supported are 2..8")
    if n * X * Y == 0 or target.numel() != n * X * Y:
        raise _lib.E2EPError(f"seg_confusion: pred {tuple(pred.shape)} vs target "
                             f"{tuple(target.shape)}")
    dev = pred.device
    with torch.no_grad():
        pred = pred.detach().contiguous()
        tg = _i64(target.detach(), dev).view(n, X * Y)
        conf = torch.empty((C, C), dtype=torch.int64, device=dev)
        ws = torch.empty(_lib.call_raw("e2ep_seg_confusion_workspace", n, X * Y),
                         dtype=torch.uint8, device=dev)
        _lib.call("e2ep_seg_confusion", _lib.ptr(pred), _lib.ptr(tg), n, C, X * Y,
                  int(ignore_index), _lib.ptr(conf), _lib.ptr(ws), _lib.nbytes(ws), _lib.stream())
    return conf


def depth_onehot(gt, d_bound, down):
    """loss/depth_loss.py:31-48 (get_down_sampled_gt_depth): min non-zero depth per down x down
    cell -> one-hot bin labels (B*N*h*w, D).  The loss itself derives the labels inside its
    kernel; this is the reference's public helper."""
    B, N, H, W = gt.shape
    D = int((d_bound[1] - d_bound[0]) / d_bound[2])
    g = gt.view(B * N, H // down, down, W // down, down, 1).permute(0, 1, 3, 5, 2, 4).contiguous()
    g = g.view(-1, down * down)
    g = torch.where(g == 0.0, 1e5 * torch.ones_like(g), g).min(-1).values
    g = (g - (d_bound[0] - d_bound[2])) / d_bound[2]
    g = torch.where((g < D + 1) & (g >= 0.0), g, torch.zeros_like(g))
    return torch.nn.functional.one_hot(g.long(), num_classes=D + 1).view(-1, D + 1)[:, 1:].float()


class _DepthBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob, gt, down, lo, step):
        prob = prob.contiguous()
        BN, D, h, w = prob.shape
        H, W = gt.shape[-2:]
        dev = prob.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        den = torch.empty(1, dtype=torch.float32, device=dev)
        cls = torch.empty(BN * h * w, dtype=torch.int32, device=dev)
        ws = _ws(_lib.load().e2ep_depth_bce_workspace(BN, H, W, down), dev)
        fn = "e2ep_depth_bce_fwd_f64" if gt.dtype == torch.float64 else "e2ep_depth_bce_fwd"
        _lib.call(fn, _lib.ptr(prob), _lib.ptr(gt), BN, D, H, W, down, lo, step,
                  _lib.ptr(loss), _lib.ptr(den), _lib.ptr(cls), _lib.ptr(ws), _lib.stream())
        ctx.save_for_backward(prob, cls, den)
        return loss

    @staticmethod
    def backward(ctx, g):
        prob, cls, den = ctx.saved_tensors
        BN, D, h, w = prob.shape
        d = torch.empty_like(prob)
        _lib.call("e2ep_depth_bce_bwd", _lib.ptr(prob), _lib.ptr(cls), _lib.ptr(den),
                  _lib.ptr(g.contiguous()), BN, D, h * w, _lib.ptr(d), _lib.stream())
        return d, None, None, None, None


def depth_bce(prob, gt, d_bound, down):
    """loss/depth_loss.py:18-28: BCE on the foreground cells, summed / max(1, #fg).
    prob (B*N, D, H/down, W/down) probabilities, gt (B, N, H, W) metric depth."""
    _dev(prob)
    B, N, H, W = gt.shape
    D = int((d_bound[1] - d_bound[0]) / d_bound[2])
    if prob.shape != (B * N, D, H // down, W // down):
        raise _lib.E2EPError(f"depth_bce: prob {tuple(prob.shape)} vs gt {tuple(gt.shape)}")
    # float64 depth (what the reference dataset yields) keeps float64 bin arithmetic; any other
    # dtype is promoted/rounded to fp32, as torch computes on a float32 tensor
    dt = torch.float64 if gt.dtype == torch.float64 else torch.float32
    g = gt.to(device=prob.device, dtype=dt, non_blocking=True).contiguous()
    lo = float(d_bound[0] - d_bound[2])  # evaluated in Python double, applied in the gt dtype
    return _DepthBCE.apply(prob, g, int(down), lo, float(d_bound[2]))


DEPTH_SUMS, DEPTH_COUNTS = 6, 5  # per camera: float64 sums and int64 counts (csrc/val.hip)


def depth_metrics_bytes(n_cams, running=False):
    """Bytes of depth_metrics' `out` buffer for n_cams cameras, or of a `running` buffer (the
    same layout followed by the int64 batch counter)."""
    return 8 * (DEPTH_SUMS + DEPTH_COUNTS) * int(n_cams) + (8 if running else 0)


def depth_metrics(prob, gt, d_bound, down, n_cams, running=None, maps=False):
    """What the depth head predicts against the ground truth, per camera, in two launches
    (csrc/val.hip; the reference only draws it: trainer/pl_trainer.py:149-168, log_depth).
    prob (B*N, D, H/down, W/down) probabilities, gt (B, N, H, W) metric depth, as depth_bce; image
    bn belongs to camera bn % n_cams.  Per foreground cell of DepthLoss (class k >= 1, true bin
    t = k - 1, g = the cell's smallest non-zero depth in metres) with a = the argmax bin,
    z_a = d_bound[0] + a * d_bound[2] (log_depth's metres, the frustum's depth of that bin) and
    z_e = the distribution's expected depth, all in float64:
        sums    |z_a - g|, (z_a - g)^2, |z_a - g| / g, |z_e - g|, (z_e - g)^2, p_t
        counts  cells, a == t, |a - t| <= 1, sum |a - t|, z_a < 1.25 g and g < 1.25 z_a
    g lies in [z_t, z_t + step), so a perfect argmax still has |z_a - g| of about step / 2.
    Returns `out`, a uint8 tensor of depth_metrics_bytes(n_cams) bytes holding this call alone:
    float64 sums[N][6] | int64 counts[N][5] (ValStep.unpack_depth reads it).  `running`, a
    zeroed uint8 tensor of depth_metrics_bytes(n_cams, running=True) bytes, has every entry of
    `out` added to it and its batch counter incremented.  maps=True returns (out, pred_map,
    gt_map, cls): z_a and g (0 for a background cell) as (B*N, H/down, W/down) fp32 and the
    class k as int32, log_depth's two panels at cell resolution.  No autograd, no host read."""
    _dev(prob, running)
    if gt.dim() != 4 or prob.dim() != 4 or prob.dtype != torch.float32:
        raise _lib.E2EPError(f"depth_metrics: prob must be (B*N, D, h, w) fp32 and gt (B, N, H, W),"
                             f" got {prob.dtype} {tuple(prob.shape)} and {tuple(gt.shape)}")
    B, N, H, W = gt.shape
    D = int((d_bound[1] - d_bound[0]) / d_bound[2])
    down, n_cams = int(down), int(n_cams)
    if down <= 0 or prob.shape != (B * N, D, H // down, W // down) or H % down or W % down:
        raise _lib.E2EPError(f"depth_metrics: prob {tuple(prob.shape)} vs gt {tuple(gt.shape)}")
    if not 1 <= n_cams <= 16 or (B * N) % n_cams:
        raise _lib.E2EPError(f"depth_metrics: {n_cams} cameras (1..16, dividing the {B * N} "
                             "images)")
    if running is not None and (running.dtype != torch.uint8 or not running.is_contiguous()
                                or running.numel() != depth_metrics_bytes(n_cams, True)):
        raise _lib.E2EPError(f"depth_metrics: running must be {depth_metrics_bytes(n_cams, True)} "
                             f"contiguous uint8 bytes for {n_cams} cameras")
    dev = prob.device
    dt = torch.float64 if gt.dtype == torch.float64 else torch.float32  # as depth_bce
    lo = float(d_bound[0] - d_bound[2])
    with torch.no_grad():
        prob = prob.detach().contiguous()
        g = gt.detach().to(device=dev, dtype=dt, non_blocking=True).contiguous()
        out = torch.empty(depth_metrics_bytes(n_cams), dtype=torch.uint8, device=dev)
        pred_map = gt_map = cls = None
        if maps:
            shape = (B * N, H // down, W // down)
            pred_map = torch.empty(shape, dtype=torch.float32, device=dev)
            gt_map = torch.empty(shape, dtype=torch.float32, device=dev)
            cls = torch.empty(shape, dtype=torch.int32, device=dev)
        ws = torch.empty(_lib.call_raw("e2ep_depth_metrics_workspace", B * N, n_cams, H, W, down),
                         dtype=torch.uint8, device=dev)
        fn = "e2ep_depth_metrics_f64" if dt == torch.float64 else "e2ep_depth_metrics"
        _lib.call(fn, _lib.ptr(prob), _lib.ptr(g), B * N, n_cams, D, H, W, down, lo,
                  float(d_bound[2]), float(d_bound[0]), float(d_bound[2]), _lib.ptr(out),
                  _lib.ptr(running), _lib.ptr(pred_map), _lib.ptr(gt_map), _lib.ptr(cls),
                  _lib.ptr(ws), _lib.nbytes(ws), _lib.stream())
    return (out, pred_map, gt_map, cls) if maps else out


ROLLOUT_SUMS, ROLLOUT_COUNTS = 4, 11  # per future frame: float64 sums and int64 counts


def rollout_metrics_bytes(F, running=False):
    """Bytes of rollout_metrics' `out` buffer for F future frames, or of a `running` buffer (the
    same layout followed by the int64 batch counter)."""
    return 8 * (ROLLOUT_SUMS + ROLLOUT_COUNTS) * int(F) + (8 if running else 0)


def rollout_metrics(seq, pred, gt_control, gt_acc, gt_steer, gt_reverse, token_nums, running=None):
    """What the free-running control decoder emits against the ground truth, per future frame,
    in two launches (csrc/val.hip).  seq (B, >= 1 + 3 F) int64, BOS first, then the decoder's own
    tokens (ParkingModel.forward_rollout; any row stride); pred (B, 3 F + 2, vocab) fp32, the
    teacher-forced logits of the same batch, or None; gt_control (B, 3 F + 3) token ids; gt_acc
    and gt_steer (B, F); gt_reverse (B, F) 0 / 1.  With p the decoded token, g the ground-truth
    one, a the argmax of pred's row and half = (token_nums - 4) / 2, per frame over the samples:
        sums    |acc_s - gt_acc|, |steer - gt_steer|, smooth_l1(acc_v, gt_acc),
                smooth_l1(steer, gt_steer)
        counts  samples, p == g for acc / steer / reverse, all three, every token up to this
                frame, (p_rev > half) == (gt_reverse == 1), any p > token_nums - 4, p == a for
                acc / steer / reverse (0 without pred)
    acc_s = p / half - 1 is the signed acceleration the agent executes (detokenize's throttle -
    brake, against the signed label), acc_v and steer are control_val's detokenisations, so the
    last two sums compare with acc_steer_val_loss.  Returns `out`, a uint8 tensor of
    rollout_metrics_bytes(F) bytes holding this call alone: float64 sums[F][4] | int64
    counts[F][11] (ValStep.unpack_rollout reads it).  `running`, a zeroed uint8 tensor of
    rollout_metrics_bytes(F, running=True) bytes, has every entry of `out` added to it and its
    batch counter incremented.  No autograd, no host read."""
    _dev(seq, running)
    if seq.dim() != 2 or seq.dtype != torch.int64 or seq.shape[1] < 4 or (seq.shape[1] - 1) % 3 \
            or (seq.shape[0] > 1 and seq.stride(0) < seq.shape[1]) or seq.stride(1) != 1:
        raise _lib.E2EPError(f"rollout_metrics: seq must be (B, 1 + 3 F) int64 with unit column "
                             f"stride, got {seq.dtype} {tuple(seq.shape)} strides {seq.stride()}")
    B, F = seq.shape[0], (seq.shape[1] - 1) // 3
    T = 3 * F + 2
    if B < 1:
        raise _lib.E2EPError("rollout_metrics: seq has no sample")
    if pred is not None:
        _dev(pred)
        if pred.dim() != 3 or pred.dtype != torch.float32 or tuple(pred.shape[:2]) != (B, T):
            raise _lib.E2EPError(f"rollout_metrics: pred must be (B, 3 F + 2, vocab) fp32 = "
                                 f"({B}, {T}, vocab), got {pred.dtype} {tuple(pred.shape)}")
    if tuple(gt_control.shape) != (B, T + 1):
        raise _lib.E2EPError(f"rollout_metrics: gt_control {tuple(gt_control.shape)} vs seq "
                             f"{tuple(seq.shape)} (expected {(B, T + 1)})")
    for name, t in (("gt_acc", gt_acc), ("gt_steer", gt_steer), ("gt_reverse", gt_reverse)):
        if tuple(t.shape) != (B, F):
            raise _lib.E2EPError(f"rollout_metrics: {name} {tuple(t.shape)} vs seq "
                                 f"{tuple(seq.shape)} (expected {(B, F)})")
    token_nums = int(token_nums)
    if token_nums < 5 or (pred is not None and pred.shape[2] != token_nums):
        raise _lib.E2EPError(f"rollout_metrics: token_nums {token_nums} (at least 5, and pred's "
                             "vocabulary)")
    if running is not None and (running.dtype != torch.uint8 or not running.is_contiguous()
                                or running.numel() != rollout_metrics_bytes(F, True)):
        raise _lib.E2EPError(f"rollout_metrics: running must be {rollout_metrics_bytes(F, True)} "
                             f"contiguous uint8 bytes for {F} frames")
    dev = seq.device
    with torch.no_grad():
        seq = seq.detach()
        pred = None if pred is None else pred.detach().contiguous()
        gtc = _i64(gt_control.detach(), dev)
        acc = gt_acc.detach().to(device=dev, dtype=torch.float32).contiguous()
        steer = gt_steer.detach().to(device=dev, dtype=torch.float32).contiguous()
        rev = _i64(gt_reverse.detach(), dev)
        out = torch.empty(rollout_metrics_bytes(F), dtype=torch.uint8, device=dev)
        ws = torch.empty(_lib.call_raw("e2ep_rollout_metrics_workspace", B, F), dtype=torch.uint8,
                         device=dev)
        _lib.call("e2ep_rollout_metrics", _lib.ptr(seq), max(seq.stride(0), seq.shape[1]),
                  _lib.ptr(pred), _lib.ptr(gtc), _lib.ptr(acc), _lib.ptr(steer), _lib.ptr(rev), B,
                  F, token_nums, token_nums - 4, _lib.ptr(out), _lib.ptr(running), _lib.ptr(ws),
                  _lib.nbytes(ws), _lib.stream())
    return out
