"""Graph-captured validation step for the ParkingModel (MI355X): TrainStep's counterpart for
the other half of an epoch.

The reference validates through PyTorch-Lightning eagerly (trainer/pl_trainer.py:85-114): the
eval forward, ControlValLoss (loss/control_loss.py:45-75, a chain of small PyTorch ops with a
synchronising .tolist() in the middle), the segmentation and depth losses, Python's sum() of
the four, and Lightning's per-epoch mean of the logged values, which
ModelCheckpoint(monitor='val_loss') selects checkpoints by.  ValStep runs

    module.parking_model(batch, noise)           the eval forward, under no_grad
    losses.control_val                           two launches (csrc/val.hip)
    seg_weighted_ce, depth_bce                   the module's loss objects (csrc/loss.hip)
    losses.seg_confusion                         two launches: the BEV head's confusion matrix
    e2ep_val_accumulate                          one launch: val_loss, and the epoch's running
                                                 sums, matrix and batch counter on the device
    losses.depth_metrics                         with depth_metrics=True, after the depth loss:
                                                 two launches, the depth head per camera
    forward_rollout, losses.rollout_metrics      with rollout=True: the forward also decodes
                                                 from BOS; two launches score the tokens

as one replayed HIP graph (graph=True) or the same calls eagerly (graph=False).  No call reads
anything back; result() makes the epoch's one device-to-host copy.

    val = ValStep(module, first_batch)           # captures; accumulates nothing yet
    for batch in loader:
        val(batch)                               # returns the batch's val_loss, a device scalar
    r = val.result()                             # {'val_loss': ..., 'seg_miou': ..., ...}
    val.reset()

Like TrainStep, graph mode captures the lift-splat plan of the construction batch's camera rig;
a batch with another rig raises.  `noise` (the (B, 2) target jitter) must be passed on every
call or on none (AgentStep's rule): without it the eval forward draws it with torch.rand, which
the captured graph replays through torch's own replay (graphs.Graph).  GEMM operand precision
(e2ep_amd.precision) is whatever is in force at the capture.

Data parallelism: each rank accumulates its own batches; result() adds the ranks' packed
buffers with one all-reduce (SUM) before it reads them, staged through the host for gloo as
TrainStep._allreduce stages the gradients.  The integer counts travel as float64 in that one
collective, exact below 2^53.

Depth metrics (depth_metrics=True): the depth head's softmax is the lift-splat weight of every
camera feature, and its BCE does not say whether a camera puts its mass in the right bin.  Per
camera and overall, over DepthLoss's foreground cells: how often the argmax bin is the true one
(depth_bin_acc, depth_bin_within1, depth_bin_mae in bins), the argmax depth z_a against the
cell's metres g (depth_abs_err, depth_rmse, depth_abs_rel, depth_delta125: the share of cells
with max(z_a / g, g / z_a) < 1.25), the distribution's expected depth against g
(depth_exp_abs_err, depth_exp_rmse) and the mass on the true bin (depth_true_bin_prob).  g lies
in [z_t, z_t + step) while a bin's depth is its lower edge z_t, so a perfect argmax still has
depth_abs_err of about step / 2.  The sums live in a second packed buffer, packed_depth, which
shares packed's allocation, copy, zeroing and all-reduce.

Rollout metrics (rollout=True): control_val scores the decoder under teacher forcing, every
position seeing the ground-truth tokens before it; the agent runs it from BOS on its own tokens
(ParkingModel.predict).  The step then runs ParkingModel.forward_rollout, which decodes every
control token of the sample beside the teacher-forced forward, and losses.rollout_metrics scores
the tokens per future frame f: rollout_acc_l1 and rollout_steer_l1 (the mean |executed value -
label|, the acceleration signed as the agent applies it), the share of samples whose acc /
steer / reverse token is the ground truth's (rollout_*_token_acc), all three
(rollout_frame_exact), every token up to and including f (rollout_prefix_exact: still on the
teacher's path), the reverse decision (rollout_reverse_acc), a decoded BOS / EOS / PAD
(rollout_invalid), and the share whose token is the teacher-forced argmax (rollout_tf_agree_*).
rollout_acc_steer_val_loss is acc_steer_val_loss's formula on the free-running tokens.  The sums
live in a third packed buffer, packed_rollout, behind the other two in the same allocation.

ParkingTrainingModule.validation_step and ControlValLoss remain as the Lightning-compatible
path; this module does not change them."""
import numpy as np
import torch
import torch.distributed as dist

from . import _lib, graphs, losses
from .train import _rig_key

KEYS = ("acc_steer_val_loss", "reverse_val_loss", "segmentation_val_loss", "depth_val_loss",
        "val_loss")  # the reference's logged names, in the packed buffer's order
_RIG = ("intrinsics", "extrinsics")
_HEAD = 8 * (len(KEYS) + 1)  # bytes of the float64 sums and the int64 batch counter
# finish_depth's keys beside depth_cells: (name, index of the numerator, 's'um or 'c'ount, sqrt)
_DEPTH = (("depth_bin_acc", 1, "c", False), ("depth_bin_within1", 2, "c", False),
          ("depth_bin_mae", 3, "c", False), ("depth_delta125", 4, "c", False),
          ("depth_abs_err", 0, "s", False), ("depth_rmse", 1, "s", True),
          ("depth_abs_rel", 2, "s", False), ("depth_exp_abs_err", 3, "s", False),
          ("depth_exp_rmse", 4, "s", True), ("depth_true_bin_prob", 5, "s", False))
# finish_rollout's per-frame keys: (name, index of the numerator, 's'um or 'c'ount)
_ROLLOUT = (("rollout_acc_l1", 0, "s"), ("rollout_steer_l1", 1, "s"),
            ("rollout_acc_token_acc", 1, "c"), ("rollout_steer_token_acc", 2, "c"),
            ("rollout_reverse_token_acc", 3, "c"), ("rollout_frame_exact", 4, "c"),
            ("rollout_prefix_exact", 5, "c"), ("rollout_reverse_acc", 6, "c"),
            ("rollout_invalid", 7, "c"), ("rollout_tf_agree_acc", 8, "c"),
            ("rollout_tf_agree_steer", 9, "c"), ("rollout_tf_agree_reverse", 10, "c"))


class ValStep:
    """One validation batch per call; see the module docstring.

    `batch`: a reference-schema batch; its tensors (the rig aside) become the step's static
    device inputs, and a later call's batch is copied into them.  `confusion=False` leaves the
    segmentation confusion matrix (and IoU) out.  `world` > 1 makes result() merge the ranks.
    `depth_metrics=True` adds the per-camera depth metrics (losses.depth_metrics) to the chain
    and to result(); `depth_maps=True` also keeps the last batch's argmax-depth, ground-truth
    and class maps at cell resolution in `self.depth_maps`.
    `rollout=True` adds the free-running decode and its metrics (losses.rollout_metrics) to the
    chain and to result(); `self.rollout_tokens` and `self.rollout_out` hold the last batch's.
    Constructing the object accumulates nothing: the warm-up runs and the capture leave the
    packed buffer zero."""

    def __init__(self, module, batch, noise=None, world=1, graph=True, warmup=2, confusion=True,
                 depth_metrics=False, depth_maps=False, rollout=False):
        p = next(module.parameters(), None)
        if p is None or not p.is_cuda:
            raise _lib.E2EPError("ValStep: the module must be on the HIP device (there is no "
                                 "host fallback)")
        _lib.load()
        self.module, self.world, self.graph = module, int(world), bool(graph)
        self.confusion = bool(confusion)
        self.device = dev = p.device
        self.batch = {k: (v.to(dev) if torch.is_tensor(v) and k not in _RIG else v)
                      for k, v in batch.items()}
        self._use_noise = noise is not None
        self.noise = noise.to(device=dev, dtype=torch.float32).clone() if self._use_noise else None
        self.C = int(module.cfg.seg_classes) if self.confusion else 0
        self.depth_metrics, self._want_maps = bool(depth_metrics), bool(depth_maps)
        if self._want_maps and not self.depth_metrics:
            raise _lib.E2EPError("ValStep: depth_maps=True needs depth_metrics=True")
        self.cams = int(self.batch["depth"].shape[1]) if self.depth_metrics else 0
        self.rollout = bool(rollout)
        self.frames = int(module.cfg.future_frame_nums) if self.rollout else 0
        if self.rollout and module.cfg.tf_de_tgt_dim != 3 * self.frames + 3:
            raise _lib.E2EPError(f"ValStep: rollout=True needs tf_de_tgt_dim = 3 * "
                                 f"future_frame_nums + 3 = {3 * self.frames + 3} (BOS, the control "
                                 f"triples, EOS, PAD), got {module.cfg.tf_de_tgt_dim}")
        n = _HEAD + 8 * self.C * self.C
        nd = losses.depth_metrics_bytes(self.cams, running=True) if self.depth_metrics else 0
        nr = losses.rollout_metrics_bytes(self.frames, running=True) if self.rollout else 0
        # one allocation, so one fill zeroes and one copy reads every packed buffer
        self._buf = torch.zeros(n + nd + nr, dtype=torch.uint8, device=dev)
        self.packed = self._buf[:n]
        self.packed_depth = self._buf[n:n + nd] if self.depth_metrics else None
        self.packed_rollout = self._buf[n + nd:] if self.rollout else None
        self._host = torch.zeros(n + nd + nr, dtype=torch.uint8).pin_memory()
        self.val_loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.pred = None  # (pred_control, pred_segmentation, pred_depth) of the last batch
        self.values = None  # device scalars of the last batch, by KEYS[:4]
        self.conf = None  # (C, C) int64 of the last batch
        self.depth_out = None  # losses.depth_metrics' buffer of the last batch
        self.depth_maps = None  # (pred_map, gt_map, cls) of the last batch, with depth_maps=True
        self.rollout_tokens = None  # (B, 1 + 3 F) int64 of the last batch, BOS first
        self.rollout_out = None  # losses.rollout_metrics' buffer of the last batch
        self._rig = _rig_key(batch)
        self._graph = None
        self._plans = []
        self.graph_memsets = 0
        if self.graph:
            self._plans = [m.prepare_capture(batch) for m in module.modules()
                           if hasattr(m, "prepare_capture")]
            self._capture(int(warmup))

    # -- the captured chain ---------------------------------------------------------------
    def _run(self):
        mod = self.module
        was_training = mod.training
        if was_training:
            mod.eval()
        try:
            with torch.no_grad():
                batch = self.batch
                toks = ro = None
                if self.rollout:
                    pc, ps, pd, toks = mod.parking_model.forward_rollout(batch, self.noise)
                else:
                    pc, ps, pd = mod.parking_model(batch, self.noise)
                ctrl = losses.control_val_out(pc, batch["gt_acc"], batch["gt_steer"],
                                              batch["gt_reverse"], mod.cfg.token_nums)
                if self.rollout:
                    ro = losses.rollout_metrics(toks, pc, batch["gt_control"], batch["gt_acc"],
                                                batch["gt_steer"], batch["gt_reverse"],
                                                mod.cfg.token_nums, running=self.packed_rollout)
                seg = mod.segmentation_loss_func(ps.unsqueeze(1), batch["segmentation"])
                depth = mod.depth_loss_func(pd, batch["depth"])
                dm = None
                if self.depth_metrics:
                    dl = mod.depth_loss_func
                    dm = losses.depth_metrics(pd, batch["depth"], dl.d_bound, dl.down_sample_factor,
                                              self.cams, running=self.packed_depth,
                                              maps=self._want_maps)
                conf = None
                if self.confusion:
                    conf = losses.seg_confusion(ps, batch["segmentation"],
                                                mod.segmentation_loss_func.ignore_index)
                _lib.call("e2ep_val_accumulate", _lib.ptr(ctrl), _lib.ptr(seg), _lib.ptr(depth),
                          _lib.ptr(conf), self.C, _lib.ptr(self.packed), _lib.ptr(self.val_loss),
                          _lib.stream())
        finally:
            if was_training:
                mod.train()
        self.pred, self.conf = (pc, ps, pd), conf
        self.rollout_tokens, self.rollout_out = toks, ro
        if self._want_maps:
            self.depth_out, self.depth_maps = dm[0], dm[1:]
        else:
            self.depth_out = dm
        self.values = {"acc_steer_val_loss": ctrl[0], "reverse_val_loss": ctrl[1],
                       "segmentation_val_loss": seg, "depth_val_loss": depth}
        return self.val_loss

    def _capture(self, warmup):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(max(warmup, 1)):  # fills every cache the capture reuses
                self._run()
            self._buf.zero_()  # the warm-up is not part of an epoch
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._graph, _, self.graph_memsets = graphs.capture(self._run)

    # -- public ---------------------------------------------------------------------------
    def __call__(self, batch=None, noise=None):
        """Validate one batch and add it to the epoch.  Returns the batch's val_loss as a
        device scalar, overwritten by the next call; nothing is read back.  A call without
        arguments runs the static inputs (batch and noise) as they are."""
        if self._use_noise != (noise is not None) and (batch is not None or noise is not None):
            raise _lib.E2EPError("ValStep: `noise` must be passed on every call or on none (the "
                                 "choice is part of the step fixed at construction)")
        if batch is not None:
            if self.graph and _rig_key(batch) != self._rig:
                raise _lib.E2EPError(
                    "ValStep(graph=True) captured the lift-splat plan of the first batch's "
                    "camera rig; this batch has different intrinsics/extrinsics (build a new "
                    "ValStep, or use graph=False, which plans every batch's rig)")
            for k, v in batch.items():
                if k in _RIG:
                    self.batch[k] = v
                elif torch.is_tensor(v) and torch.is_tensor(self.batch.get(k)):
                    self.batch[k].copy_(v, non_blocking=True)
        if noise is not None:
            self.noise.copy_(noise, non_blocking=True)
        if self._graph is not None:
            self._graph.replay()
            return self.val_loss
        return self._run()

    def reset(self):
        """Start an epoch: zero the running sums, the confusion matrix and the counter (and the
        depth and rollout metrics' packed buffers, which share the allocation)."""
        self._buf.zero_()

    def _merge(self):
        """The ranks' packed buffers added into a host copy: one all-reduce (SUM), the counts
        as float64 beside the sums (once per epoch, outside the captured chain: the RCCL path
        forms that vector with two small torch ops on the device)."""
        return self._merge_all()[0]

    def _merge_all(self):
        """_merge for both packed buffers, (packed, packed_depth or None): the depth metrics'
        sums and counts ride behind the others in the same all-reduce."""
        return self._merge_every()[:2]

    def _merge_every(self):
        """_merge for the three packed buffers, (packed, packed_depth or None, packed_rollout
        or None): the rollout metrics' sums and counts ride behind the depth metrics'."""
        ns = self.cams * losses.DEPTH_SUMS  # float64 sums at the head of packed_depth
        nrs = self.frames * losses.ROLLOUT_SUMS  # and of packed_rollout
        n0, n1 = self.packed.numel(), self._buf.numel() - (self.packed_rollout.numel()
                                                           if self.rollout else 0)
        if dist.get_backend() == "nccl":
            sums = self.packed[:_HEAD - 8].view(torch.float64)
            counts = self.packed[_HEAD - 8:].view(torch.int64)
            parts = [sums, counts.to(torch.float64)]
            if self.depth_metrics:
                parts += [self.packed_depth[:8 * ns].view(torch.float64),
                          self.packed_depth[8 * ns:].view(torch.int64).to(torch.float64)]
            if self.rollout:
                parts += [self.packed_rollout[:8 * nrs].view(torch.float64),
                          self.packed_rollout[8 * nrs:].view(torch.int64).to(torch.float64)]
            flat = torch.cat(parts)
            dist.all_reduce(flat)
            flat = flat.cpu()
        else:  # gloo: staged through the host, the ordering explicit
            self._host.copy_(self._buf, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            host = self._host.numpy()
            sums, batches, conf = self.unpack(host[:n0])
            counts = np.concatenate([[batches], conf.reshape(-1) if conf is not None else []])
            parts = [sums, counts.astype(np.float64)]
            if self.depth_metrics:
                dsums, dcounts, dbatches = self.unpack_depth(host[n0:n1])
                parts += [dsums.reshape(-1), dcounts.reshape(-1).astype(np.float64),
                          np.asarray([dbatches], dtype=np.float64)]
            if self.rollout:
                rsums, rcounts, rbatches = self.unpack_rollout(host[n1:])
                parts += [rsums.reshape(-1), rcounts.reshape(-1).astype(np.float64),
                          np.asarray([rbatches], dtype=np.float64)]
            flat = torch.from_numpy(np.concatenate(parts))
            dist.all_reduce(flat)
        flat = flat.numpy()
        n, cells = len(KEYS), self.C * self.C
        conf = (np.rint(flat[n + 1:n + 1 + cells]).astype(np.int64).reshape(self.C, self.C)
                if self.C else None)
        packed = self.pack(flat[:n], int(round(flat[n])), conf)
        packed_depth = packed_rollout = None
        d = flat[n + 1 + cells:]
        if self.depth_metrics:
            nd = self.cams * (losses.DEPTH_SUMS + losses.DEPTH_COUNTS) + 1
            dcounts = np.rint(d[ns:nd]).astype(np.int64)
            packed_depth = self.pack_depth(d[:ns].reshape(self.cams, -1),
                                           dcounts[:-1].reshape(self.cams, -1), int(dcounts[-1]))
            d = d[nd:]
        if self.rollout:
            rcounts = np.rint(d[nrs:]).astype(np.int64)
            packed_rollout = self.pack_rollout(d[:nrs].reshape(self.frames, -1),
                                               rcounts[:-1].reshape(self.frames, -1),
                                               int(rcounts[-1]))
        return packed, packed_depth, packed_rollout

    def result(self):
        """The epoch so far: one device-to-host copy (after one all-reduce when world > 1),
        then finish(), and with depth_metrics=True finish_depth() and with rollout=True
        finish_rollout() merged into the same dict."""
        if self.world > 1:
            packed, packed_depth, packed_rollout = self._merge_every()
        else:
            self._host.copy_(self._buf, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            host = self._host.numpy().copy()
            n0 = self.packed.numel()
            n1 = host.size - (self.packed_rollout.numel() if self.rollout else 0)
            packed, packed_depth, packed_rollout = host[:n0], host[n0:n1], host[n1:]
        out = self.finish(packed)
        if self.depth_metrics:
            out.update(self.finish_depth(packed_depth))
        if self.rollout:
            out.update(self.finish_rollout(packed_rollout))
        return out

    # -- host arithmetic on the packed buffer ------------------------------------------------
    @staticmethod
    def pack(sums, batches, conf=None):
        """The packed buffer's bytes (uint8 array) from five float64 sums, the batch count and
        the (C, C) int64 running confusion matrix (or None)."""
        sums = np.asarray(sums, dtype=np.float64).reshape(len(KEYS))
        tail = np.asarray([] if conf is None else conf, dtype=np.int64).reshape(-1)
        counts = np.concatenate([np.asarray([batches], dtype=np.int64), tail])
        return np.concatenate([sums.view(np.uint8), counts.view(np.uint8)])

    @staticmethod
    def unpack(packed):
        """(sums float64 [5], batches int, conf int64 (C, C) or None) of a packed buffer."""
        raw = np.ascontiguousarray(np.asarray(packed, dtype=np.uint8).reshape(-1))
        cells = (raw.size - _HEAD) // 8
        C = int(round(cells ** 0.5))
        if raw.size < _HEAD or raw.size != _HEAD + 8 * C * C:
            raise _lib.E2EPError(f"ValStep: {raw.size} bytes are no packed validation buffer")
        sums = raw[:_HEAD - 8].view(np.float64).copy()
        counts = raw[_HEAD - 8:].view(np.int64)
        return sums, int(counts[0]), (counts[1:].reshape(C, C).copy() if C else None)

    @staticmethod
    def finish(packed):
        """Epoch results from a packed buffer's bytes, on the host: the five reference keys as
        means over the batches (float64; NaN without a batch), `batches`, and with a confusion
        matrix `seg_confusion` (rows = target, columns = prediction), `seg_iou` per class
        (intersection / union, NaN for a class that occurs in neither) and `seg_miou` (the
        mean over the classes that occur)."""
        sums, batches, conf = ValStep.unpack(packed)
        out = {k: (float(s) / batches if batches else float("nan")) for k, s in zip(KEYS, sums)}
        out["batches"] = batches
        if conf is not None:
            inter = np.diag(conf).astype(np.float64)
            union = (conf.sum(1) + conf.sum(0)).astype(np.float64) - inter
            iou = np.full(len(inter), np.nan)
            np.divide(inter, union, out=iou, where=union > 0)
            out["seg_confusion"] = conf
            out["seg_iou"] = iou
            out["seg_miou"] = float(iou[union > 0].mean()) if (union > 0).any() else float("nan")
        return out

    @staticmethod
    def pack_depth(sums, counts, batches):
        """The depth metrics' packed buffer (uint8 array) from the (N, 6) float64 sums, the
        (N, 5) int64 counts (losses.depth_metrics' order) and the batch count."""
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        N = sums.shape[0] if sums.ndim == 2 else -1
        if (N < 1 or sums.shape != (N, losses.DEPTH_SUMS)
                or counts.shape != (N, losses.DEPTH_COUNTS)):
            raise _lib.E2EPError(f"ValStep: depth sums {sums.shape} and counts {counts.shape} are "
                                 f"not (N, {losses.DEPTH_SUMS}) and (N, {losses.DEPTH_COUNTS})")
        tail = np.asarray([batches], dtype=np.int64)
        return np.concatenate([sums.reshape(-1).view(np.uint8), counts.reshape(-1).view(np.uint8),
                               tail.view(np.uint8)])

    @staticmethod
    def unpack_depth(packed_depth):
        """(sums float64 (N, 6), counts int64 (N, 5), batches int) of a depth packed buffer; of
        one batch's `depth_out` (no counter behind it) batches is None."""
        raw = np.ascontiguousarray(np.asarray(packed_depth, dtype=np.uint8).reshape(-1))
        per = losses.depth_metrics_bytes(1)
        N, rest = divmod(raw.size, per)
        if N < 1 or rest not in (0, 8):
            raise _lib.E2EPError(f"ValStep: {raw.size} bytes are no packed depth-metrics buffer")
        ns = 8 * N * losses.DEPTH_SUMS
        sums = raw[:ns].view(np.float64).reshape(N, -1).copy()
        counts = raw[ns:N * per].view(np.int64).reshape(N, -1).copy()
        return sums, counts, (int(raw[N * per:].view(np.int64)[0]) if rest else None)

    @staticmethod
    def finish_depth(packed_depth):
        """Epoch results of the depth metrics from their packed buffer's bytes, on the host:
        depth_cells and the ten ratios of the module docstring over all cameras (the cameras'
        sums added in order), and `depth_per_camera`, the same keys as arrays of length N.  A
        ratio is NaN where there is no cell."""
        sums, counts, _ = ValStep.unpack_depth(packed_depth)

        def ratios(s, c):
            cells = c[..., 0].astype(np.float64)
            out = {"depth_cells": c[..., 0].copy()}
            for key, i, kind, root in _DEPTH:
                num = (s if kind == "s" else c)[..., i].astype(np.float64)
                v = np.full(cells.shape, np.nan)
                np.divide(num, cells, out=v, where=cells > 0)
                out[key] = np.sqrt(v) if root else v
            return out

        total_s = np.zeros(losses.DEPTH_SUMS)
        for row in sums:
            total_s = total_s + row
        out = {k: (int(v) if k == "depth_cells" else float(v))
               for k, v in ratios(total_s, counts.sum(0)).items()}
        out["depth_per_camera"] = ratios(sums, counts)
        return out

    @staticmethod
    def pack_rollout(sums, counts, batches):
        """The rollout metrics' packed buffer (uint8 array) from the (F, 4) float64 sums, the
        (F, 11) int64 counts (losses.rollout_metrics' order) and the batch count."""
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        F = sums.shape[0] if sums.ndim == 2 else -1
        if (F < 1 or sums.shape != (F, losses.ROLLOUT_SUMS)
                or counts.shape != (F, losses.ROLLOUT_COUNTS)):
            raise _lib.E2EPError(f"ValStep: rollout sums {sums.shape} and counts {counts.shape} "
                                 f"are not (F, {losses.ROLLOUT_SUMS}) and "
                                 f"(F, {losses.ROLLOUT_COUNTS})")
        tail = np.asarray([batches], dtype=np.int64)
        return np.concatenate([sums.reshape(-1).view(np.uint8), counts.reshape(-1).view(np.uint8),
                               tail.view(np.uint8)])

    @staticmethod
    def unpack_rollout(packed_rollout):
        """(sums float64 (F, 4), counts int64 (F, 11), batches int) of a rollout packed buffer;
        of one batch's `rollout_out` (no counter behind it) batches is None."""
        raw = np.ascontiguousarray(np.asarray(packed_rollout, dtype=np.uint8).reshape(-1))
        per = losses.rollout_metrics_bytes(1)
        F, rest = divmod(raw.size, per)
        if F < 1 or rest not in (0, 8):
            raise _lib.E2EPError(f"ValStep: {raw.size} bytes are no packed rollout-metrics buffer")
        ns = 8 * F * losses.ROLLOUT_SUMS
        sums = raw[:ns].view(np.float64).reshape(F, -1).copy()
        counts = raw[ns:F * per].view(np.int64).reshape(F, -1).copy()
        return sums, counts, (int(raw[F * per:].view(np.int64)[0]) if rest else None)

    @staticmethod
    def finish_rollout(packed_rollout):
        """Epoch results of the rollout metrics from their packed buffer's bytes, on the host:
        the twelve per-frame ratios of the module docstring as float64 arrays of length F (each
        numerator over the frame's samples, NaN where there is none), `rollout_samples`, and
        `rollout_acc_steer_val_loss`: the mean over every (sample, frame) of the acc SmoothL1
        plus that of the steer one, acc_steer_val_loss's formula on the free-running tokens (the
        frames' sums added in order)."""
        sums, counts, _ = ValStep.unpack_rollout(packed_rollout)
        samples = counts[:, 0].astype(np.float64)
        out = {}
        for key, i, kind in _ROLLOUT:
            num = (sums if kind == "s" else counts)[:, i].astype(np.float64)
            v = np.full(samples.shape, np.nan)
            np.divide(num, samples, out=v, where=samples > 0)
            out[key] = v
        acc = steer = 0.0
        for row in sums:
            acc, steer = acc + row[2], steer + row[3]
        n = float(samples.sum())
        out["rollout_acc_steer_val_loss"] = (float(acc) / n + float(steer) / n if n
                                             else float("nan"))
        out["rollout_samples"] = int(counts[0, 0])
        return out
