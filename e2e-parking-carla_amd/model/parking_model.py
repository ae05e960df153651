"""ParkingModel — MI355X-native drop-in for reference model/parking_model.py:12-78.

Same constructor (`ParkingModel(cfg)`), submodules (bev_model, bev_encoder, feature_fusion,
control_predict, segmentation_head), state-dict keys (861) and methods (forward, predict,
encoder, add_target_bev).  Differences are internal: the lift-splat pooling writes straight
into a 65-channel BEV buffer whose last plane the target-point kernel fills, so the
reference's torch.cat of the target channel (:45) and its per-sample Python loop (:39-43)
disappear.  `noise` (optional, (B,2) in [0,1)) replaces the torch.rand_like draw (:36) for
reproducible runs; by default it is drawn on the device exactly like the reference."""
import torch
from torch import nn

from e2ep_amd import _lib, conv, lss, nn_ops, rng, segments, streams
from model.bev_encoder import BevEncoder
from model.bev_model import BevModel
from model.control_predict import ControlPredict
from model.feature_fusion import FeatureFusion
from model.segmentation_head import SegmentationHead


class ParkingModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.bev_model = BevModel(self.cfg)
        self.bev_encoder = BevEncoder(self.cfg.bev_encoder_in_channel)
        self.feature_fusion = FeatureFusion(self.cfg)
        self.control_predict = ControlPredict(self.cfg)
        self.segmentation_head = SegmentationHead(self.cfg)

    def _noise(self, b, device, noise):
        if noise is None:  # the step's uniform pool inside a training forward (e2ep_amd.rng)
            return rng.uniform((b, 2), device)
        return noise

    def add_target_bev(self, bev_feature, target_point, noise=None):
        """Append the target-point channel to a (B,C,X,Y) BEV tensor (reference API)."""
        b, c, h, w = bev_feature.shape
        out = torch.empty((b, c + 1, h, w), dtype=bev_feature.dtype, device=bev_feature.device)
        out[:, :c] = bev_feature
        lss.target_bev(out, c, target_point, self._noise(b, out.device, noise),
                       self.cfg.bev_x_bound[2], self.cfg.bev_y_bound[2])
        return out, out[:, c:].detach().clone()

    def encoder(self, data, noise=None):
        """(fuse_feature, pred_segmentation, pred_depth, bev_target) — reference API."""
        out, br = self._encoder_async(data, noise)
        return (out[0], br.join(out[1]), out[2], out[3])

    def _encoder_async(self, data, noise=None):
        """encoder() whose segmentation head may still be running on a side stream (branch
        "heads", e2ep_amd.streams): returns (outputs, branch); branch.join(pred_segmentation)
        before using it.  forward() / predict() run the control decoder in between."""
        # every spatial conv weight's tap-major copy in one launch (e2ep_amd.conv.TapMajorBatch)
        if getattr(self, "_tap_batch", None) is None:
            self._tap_batch = conv.TapMajorBatch()
        with self._tap_batch:
            if self.training:  # all BN num_batches_tracked updates in one launch
                if getattr(self, "_bn_counters", None) is None:
                    self._bn_counters = nn_ops.BnCounters()
                with self._bn_counters:
                    return self._encoder(data, noise)
            # inference: the fused BN consumers' eval statistics in one launch (no_grad only)
            if getattr(self, "_eval_bn", None) is None:
                self._eval_bn = nn_ops.EvalBnBatch()
            with self._eval_bn:
                return self._encoder(data, noise)

    def _encoder(self, data, noise=None):
        dev = self.bev_model.frustum.device
        images = data["image"].to(dev, non_blocking=True)
        target_point = data["target_point"].to(dev, non_blocking=True)
        ego_motion = data["ego_motion"].to(dev, non_blocking=True)
        b = images.shape[0]
        bev, pred_depth = self.bev_model.calc_bev_feature(images, data["intrinsics"],
                                                          data["extrinsics"])
        # segment boundary of the data-parallel captured step (e2ep_amd.segments; identity
        # otherwise): everything below (camera encoder, lift-splat) backpropagates in stage 2
        bev, pred_depth = segments.cut(bev), segments.cut(pred_depth)
        # target plane (model/parking_model.py:28-46) as its own constant tensor; the BEV
        # encoder stem consumes (bev, target) without materialising their concatenation
        X, Y = bev.shape[-2:]
        bev_target = torch.empty((b, 1, X, Y), dtype=torch.float32, device=dev)
        lss.target_bev(bev_target, 0, target_point, self._noise(b, dev, noise),
                       self.cfg.bev_x_bound[2], self.cfg.bev_y_bound[2])
        bev_down_sample = self.bev_encoder.forward_split(bev, bev_target)
        fuse_feature = self.feature_fusion(bev_down_sample, ego_motion)
        # fuse_feature feeds the segmentation head and the control decoder (nn_ops.fork2); the
        # segmentation head (a few large 200x200 launches) runs on a side stream next to the
        # control decoder (a chain of small token-row launches)
        fuse_seg, fuse_feature = nn_ops.fork2(fuse_feature)
        br = streams.branch("heads", dev, (fuse_seg,), self.training)
        with br:
            pred_segmentation = self.segmentation_head(fuse_seg)
        return (fuse_feature, pred_segmentation, pred_depth, bev_target), br

    def forward(self, data, noise=None):
        if self.training:  # one launch draws every dropout seed of this step (e2ep_amd.rng)
            rng.begin_step(data["image"].device)
        try:
            (fuse_feature, pred_segmentation, pred_depth, _), br = self._encoder_async(data, noise)
            gt = data["gt_control"].to(fuse_feature.device, non_blocking=True)
            pred_control = self.control_predict(fuse_feature, gt)
            pred_segmentation = br.join(pred_segmentation)
        finally:
            if self.training:
                rng.end_step()
        return pred_control, pred_segmentation, pred_depth

    def forward_rollout(self, data, noise=None, steps=None):
        """forward() plus the free-running decode of the same sample: (pred_control,
        pred_segmentation, pred_depth, rollout_tokens).  The three predictions are forward()'s;
        rollout_tokens (B, 1 + steps) int64 is what predict()'s loop emits from BOS
        (gt_control[:, :1]) when the decoder is fed its own tokens, BOS first: a view of the
        decode's (B, tf_de_tgt_dim - 1) buffer, so its row stride is that width.  `steps`
        defaults to 3 * future_frame_nums, every control token of the sample.  The decode runs
        between the teacher-forced decoder and the join of the segmentation head's side stream.
        Where ar_decode.eligible holds (fp32 linears, B <= 16, no hooks) it is the KV-cached
        incremental decode; elsewhere predict_tokens runs its full pass per token, as for
        predict(): the same tokens.  Eval and no_grad only (validation: e2ep_amd.val)."""
        if self.training:
            raise _lib.E2EPError("ParkingModel.forward_rollout: eval mode only (the rollout is a "
                                 "validation metric; call .eval() first)")
        steps = 3 * self.cfg.future_frame_nums if steps is None else int(steps)
        with torch.no_grad():
            (fuse_feature, pred_segmentation, pred_depth, _), br = self._encoder_async(data, noise)
            gt = data["gt_control"].to(fuse_feature.device, non_blocking=True)
            pred_control = self.control_predict(fuse_feature, gt)
            rollout_tokens = self.control_predict.predict_tokens(fuse_feature, gt[:, :1], steps)
            pred_segmentation = br.join(pred_segmentation)
        return pred_control, pred_segmentation, pred_depth, rollout_tokens

    def predict(self, data, noise=None):
        (fuse_feature, pred_segmentation, pred_depth, bev_target), br = self._encoder_async(data, noise)
        toks = data["gt_control"].to(fuse_feature.device, non_blocking=True)
        # three predict() calls, each appending its token (reference :72-78), on one token
        # buffer: two e2ep launches for the padding / softmax / argmax / cat of all three
        toks = self.control_predict.predict_tokens(fuse_feature, toks, 3)
        return toks, br.join(pred_segmentation), pred_depth, bev_target
