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


class ValStep:
    """One validation batch per call; see the module docstring.

    `batch`: a reference-schema batch; its tensors (the rig aside) become the step's static
    device inputs, and a later call's batch is copied into them.  `confusion=False` leaves the
    segmentation confusion matrix (and IoU) out.  `world` > 1 makes result() merge the ranks.
    Constructing the object accumulates nothing: the warm-up runs and the capture leave the
    packed buffer zero."""

    def __init__(self, module, batch, noise=None, world=1, graph=True, warmup=2, confusion=True):
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
        self.packed = torch.zeros(_HEAD + 8 * self.C * self.C, dtype=torch.uint8, device=dev)
        self._host = torch.zeros(self.packed.numel(), dtype=torch.uint8).pin_memory()
        self.val_loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.pred = None  # (pred_control, pred_segmentation, pred_depth) of the last batch
        self.values = None  # device scalars of the last batch, by KEYS[:4]
        self.conf = None  # (C, C) int64 of the last batch
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
                pc, ps, pd = mod.parking_model(batch, self.noise)
                ctrl = losses.control_val_out(pc, batch["gt_acc"], batch["gt_steer"],
                                              batch["gt_reverse"], mod.cfg.token_nums)
                seg = mod.segmentation_loss_func(ps.unsqueeze(1), batch["segmentation"])
                depth = mod.depth_loss_func(pd, batch["depth"])
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
        self.values = {"acc_steer_val_loss": ctrl[0], "reverse_val_loss": ctrl[1],
                       "segmentation_val_loss": seg, "depth_val_loss": depth}
        return self.val_loss

    def _capture(self, warmup):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(max(warmup, 1)):  # fills every cache the capture reuses
                self._run()
            self.packed.zero_()  # the warm-up is not part of an epoch
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
        """Start an epoch: zero the running sums, the confusion matrix and the counter."""
        self.packed.zero_()

    def _merge(self):
        """The ranks' packed buffers added into a host copy: one all-reduce (SUM), the counts
        as float64 beside the sums (once per epoch, outside the captured chain: the RCCL path
        forms that vector with two small torch ops on the device)."""
        if dist.get_backend() == "nccl":
            sums = self.packed[:_HEAD - 8].view(torch.float64)
            counts = self.packed[_HEAD - 8:].view(torch.int64)
            flat = torch.cat([sums, counts.to(torch.float64)])
            dist.all_reduce(flat)
            flat = flat.cpu()
        else:  # gloo: staged through the host, the ordering explicit
            self._host.copy_(self.packed, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            sums, batches, conf = self.unpack(self._host.numpy())
            counts = np.concatenate([[batches], conf.reshape(-1) if conf is not None else []])
            flat = torch.from_numpy(np.concatenate([sums, counts.astype(np.float64)]))
            dist.all_reduce(flat)
        flat = flat.numpy()
        n = len(KEYS)
        conf = np.rint(flat[n + 1:]).astype(np.int64).reshape(self.C, self.C) if self.C else None
        return self.pack(flat[:n], int(round(flat[n])), conf)

    def result(self):
        """The epoch so far: one device-to-host copy (after one all-reduce when world > 1),
        then finish()."""
        if self.world > 1:
            return self.finish(self._merge())
        self._host.copy_(self.packed, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self.finish(self._host.numpy().copy())

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
