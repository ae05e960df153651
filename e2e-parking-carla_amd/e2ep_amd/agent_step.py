"""The closed-loop agent's tick on the device: raw sensor frames in, controls and the fed-back
target point out (csrc/agent.hip, csrc/decode.hip).

The reference agent (agent/parking_agent.py) wraps every ParkingModel.predict in host work:
four ProcessImage calls, torch.cat and an fp32 H2D before it (get_model_data :458-476); after
it torch.argmax, a synchronising .cpu(), a Python loop over all 40 000 BEV pixels for the
target slot's centroid (save_prev_target :290-311, get_target_point_ego_coord :313-318), the
next frame's target_point[:2], and detokenize (:391).  AgentStep.tick replaces that chain by

    one H2D (raw uint8 BGRA frames + ego motion, goal and noise)
    decode_bgra -> target_select -> model.predict -> slot_partials + slot_finish
        (a replayed HIP graph, or the same calls run eagerly with capture=False)
    one D2H of the packed result (a few dozen bytes), one stream synchronisation

with the fed-back target point kept in device memory between ticks.  The functions below are
the thin bindings of the four entry points; every result is bit-identical to the host chain.
There is no host fallback: CPU tensors raise."""
import ctypes

import numpy as np
import torch

from . import _lib, graphs

CLASS_LUT = (0, 128, 255)  # save_seg_img's grey levels (agent/parking_agent.py:276-277)


def _dev(t, name, dtype):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.E2EPError(f"agent_step: {name} must be a tensor on the HIP device (there is "
                             "no host fallback)")
    if t.dtype != dtype:
        raise _lib.E2EPError(f"agent_step: {name} must be {dtype}, got {t.dtype}")


def _dense(t, name, dtype, shape=None):
    _dev(t, name, dtype)
    if not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise _lib.E2EPError(f"agent_step: {name} must be contiguous"
                             + (f" {tuple(shape)}" if shape is not None else "")
                             + f", got {tuple(t.shape)}")


def decode_bgra(bgra, crop, out_image=None, out_rgb=None, rgb=False):
    """(N, H, W, 4) uint8 BGRA frames on the device -> (image (N, 3, crop, crop) fp32, exactly
    ProcessImage's; the (N, crop, crop, 3) uint8 RGB crop when `rgb` or out_rgb, else None)."""
    _dense(bgra, "bgra", torch.uint8)
    if bgra.dim() != 4 or bgra.shape[-1] != 4:
        raise _lib.E2EPError(f"decode_bgra: frames must be (N, H, W, 4), got {tuple(bgra.shape)}")
    N, H, W = bgra.shape[:3]
    crop = int(crop)
    image = out_image if out_image is not None else torch.empty(
        (N, 3, max(crop, 0), max(crop, 0)), dtype=torch.float32, device=bgra.device)
    _dense(image, "out_image", torch.float32, (N, 3, crop, crop))
    if out_rgb is None and rgb:
        out_rgb = torch.empty((N, crop, crop, 3), dtype=torch.uint8, device=bgra.device)
    if out_rgb is not None:
        _dense(out_rgb, "out_rgb", torch.uint8, (N, crop, crop, 3))
    _lib.call("e2ep_decode_bgra", _lib.ptr(bgra), N, H, W, crop, _lib.ptr(image),
              _lib.ptr(out_rgb), _lib.stream())
    return image, out_rgb


def slot_workspace(B, X, device):
    """The int32 partials buffer of slot_stats for (B, *, X, *) logits."""
    n = _lib.call_raw("e2ep_slot_stats_workspace", int(B), int(X))
    return torch.empty(max(n // 4, 1), dtype=torch.int32, device=device)


def new_state(B, device):
    """The persistent per-sample (valid, px, py) state, cleared."""
    return torch.zeros((B, 3), dtype=torch.float32, device=device)


def slot_stats(logits, state, res, target_class=2, workspace=None, class_image=None,
               class_lut=CLASS_LUT, found=None, stats=None, seq=None, first=1, token_nums=204,
               controls=None, tokens_out=None):
    """Two launches: the target-class centroid of (B, C, X, Y) logits (any strides) into
    `state` (B, 3) — untouched where the class has no pixel — and, with `seq`, the detokenized
    controls of seq[:, first:first + 3].  `res` = (bev_x_bound[2], bev_y_bound[2]).  Optional
    outputs: class_image (B, X, Y) uint8 (flipped, through class_lut), found (B,) int32,
    stats (B, 3) int64 (count, tx, ty), controls (B, 4) float64, tokens_out (B, seq.shape[1])
    int64.  Returns the workspace used."""
    _dev(logits, "logits", torch.float32)
    if logits.dim() != 4:
        raise _lib.E2EPError(f"slot_stats: logits must be (B, C, X, Y), got {tuple(logits.shape)}")
    B, C, X, Y = logits.shape
    _dense(state, "state", torch.float32, (B, 3))
    if workspace is None:
        workspace = slot_workspace(B, X, logits.device)
    _dense(workspace, "workspace", torch.int32)
    lut = None
    if class_image is not None:
        _dense(class_image, "class_image", torch.uint8, (B, X, Y))
        if len(class_lut) < C:
            raise _lib.E2EPError(f"slot_stats: class_lut holds {len(class_lut)} values for {C} classes")
        lut = (ctypes.c_ubyte * C)(*[int(v) for v in class_lut[:C]])
    if found is not None:
        _dense(found, "found", torch.int32, (B,))
    if stats is not None:
        _dense(stats, "stats", torch.int64, (B, 3))
    sb, sc, sx, sy = logits.stride()
    _lib.call("e2ep_slot_partials", _lib.ptr(logits), sb, sc, sx, sy, B, C, X, Y,
              int(target_class), lut, _lib.ptr(class_image), _lib.ptr(workspace),
              _lib.nbytes(workspace), _lib.stream())
    stride = length = 0
    if seq is not None:
        _dev(seq, "seq", torch.int64)
        if seq.dim() != 2 or seq.shape[0] != B or seq.stride(1) != 1:
            raise _lib.E2EPError(f"slot_stats: seq must be (B, T) int64 rows, got {tuple(seq.shape)}")
        stride, length = seq.stride(0), seq.shape[1]
        if controls is not None:
            _dense(controls, "controls", torch.float64, (B, 4))
        if tokens_out is not None:
            _dense(tokens_out, "tokens_out", torch.int64, (B, length))
    _lib.call("e2ep_slot_finish", _lib.ptr(workspace), _lib.nbytes(workspace), B, X, Y,
              float(res[0]), float(res[1]), _lib.ptr(state), _lib.ptr(found), _lib.ptr(stats),
              _lib.ptr(seq), stride, length, int(first), int(token_nums),
              _lib.ptr(controls if seq is not None else None),
              _lib.ptr(tokens_out if seq is not None else None), _lib.stream())
    return workspace


def target_select(state, goal, out=None):
    """get_model_data's choice (agent/parking_agent.py:474-476): (px, py, goal yaw) of the
    samples whose state is valid, the goal elsewhere.  goal (B, 3) fp32."""
    _dev(goal, "goal", torch.float32)
    B = goal.shape[0]
    _dense(goal, "goal", torch.float32, (B, 3))
    _dense(state, "state", torch.float32, (B, 3))
    if out is None:
        out = torch.empty_like(goal)
    _dense(out, "out", torch.float32, (B, 3))
    _lib.call("e2ep_target_select", _lib.ptr(state), _lib.ptr(goal), B, _lib.ptr(out),
              _lib.stream())
    return out


class TickResult:
    """controls [throttle, brake, steer, reverse]; tokens (the predicted row, prefix
    included); target_point_used (x, y, yaw fed to the model); slot_found; next_target
    ((x, y) the next tick will use, or None while no slot has been found since reset())."""
    __slots__ = ("controls", "tokens", "target_point_used", "slot_found", "next_target",
                 "slot_stats")

    def __repr__(self):
        return ("TickResult(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")")


def _align(n, a=16):
    return -(-n // a) * a


def _rig_key(k, e):
    k, e = k.detach().float().cpu().contiguous(), e.detach().float().cpu().contiguous()
    return (tuple(k.shape), tuple(e.shape), k.numpy().tobytes(), e.numpy().tobytes())


class AgentStep:
    """One agent tick (B = 1) around `model.predict`, see the module docstring.

        step = AgentStep(model, cam_hw=(300, 400))      # a ParkingModel on the HIP device
        r = step.tick(frames, ego_motion, goal_target_point, intrinsics, extrinsics)
        control.throttle, control.brake, control.steer, control.reverse = r.controls

    `frames`: uint8 (n_cams, H, W, 4) BGRA array / tensor, or a list of n_cams sensor images
    with `raw_data`, `height`, `width`.  The first tick fixes the camera rig and whether
    `noise` is passed; with capture=True it runs the chain eagerly once, captures it into a
    HIP graph and replays that graph from then on.  A later tick with a different rig raises
    (TrainStep's rule): the captured lift-splat plan is never silently replanned.  GEMM operand
    precision (e2ep_amd.precision) and forward hooks on the model are those in force at the
    first tick; a hook's output tensor is a static output of the graph.

    Device tensors of the last tick: pred_segmentation, target_bev, image; with display=True
    also seg_image (uint8 (1, X, Y), flipped, 0 / 128 / 255) and rgb_crops (n_cams, crop, crop,
    3)."""

    def __init__(self, model, cam_hw=(300, 400), n_cams=4, token_prefix=1, capture=True,
                 display=False):
        p = next(model.parameters(), None)
        if p is None or not p.is_cuda:
            raise _lib.E2EPError("AgentStep: the model must be on the HIP device (there is no "
                                 "host fallback)")
        _lib.load()
        self.model, self.cfg, self.device = model, model.cfg, p.device
        self.H, self.W = int(cam_hw[0]), int(cam_hw[1])
        self.n_cams, self.prefix = int(n_cams), int(token_prefix)
        self.crop = int(self.cfg.image_crop)
        if self.crop > self.H or self.crop > self.W:
            raise _lib.E2EPError(f"AgentStep: image_crop {self.crop} exceeds the {self.H} x "
                                 f"{self.W} camera frame")
        if self.prefix < 1:
            raise _lib.E2EPError("AgentStep: token_prefix must be >= 1 (the BOS token)")
        self.capture, self.display = bool(capture), bool(display)
        self.res = (float(self.cfg.bev_x_bound[2]), float(self.cfg.bev_y_bound[2]))
        dev = self.device
        # input: frames | ego motion (3) | goal (3) | noise (2), one pinned + one device buffer
        nf = self.n_cams * self.H * self.W * 4
        self._off = _align(nf)
        self._in_host = torch.zeros(self._off + 32, dtype=torch.uint8).pin_memory()
        self._in_dev = torch.zeros(self._off + 32, dtype=torch.uint8, device=dev)
        shape = (self.n_cams, self.H, self.W, 4)
        self._frames_host = self._in_host[:nf].view(shape)
        self._sc_host = self._in_host[self._off:].view(torch.float32)
        self.frames = self._in_dev[:nf].view(shape)
        sc = self._in_dev[self._off:].view(torch.float32)
        self._ego, self._goal, self._noise = sc[0:3].view(1, 1, 3), sc[3:6].view(1, 3), sc[6:8].view(1, 2)
        # result: controls f64 (4) | tokens i64 (T) | stats i64 (3) | target used f32 (3) |
        # state f32 (3) | found i32 (1); the state persists here between ticks
        T = self.T = self.prefix + 3
        n = 32 + 8 * T + 24 + 12 + 12 + 4
        self._out_dev = torch.zeros(_align(n), dtype=torch.uint8, device=dev)
        self._out_host = torch.zeros(_align(n), dtype=torch.uint8).pin_memory()

        def carve(buf):
            o = [0]

            def take(nbytes, dtype, shape):
                v = buf[o[0]:o[0] + nbytes].view(dtype).view(shape)
                o[0] += nbytes
                return v
            return (take(32, torch.float64, (1, 4)), take(8 * T, torch.int64, (1, T)),
                    take(24, torch.int64, (1, 3)), take(12, torch.float32, (1, 3)),
                    take(12, torch.float32, (1, 3)), take(4, torch.int32, (1,)))
        (self._controls, self._tokens, self._stats, self.target_point_used, self.state,
         self._found) = carve(self._out_dev)
        self._h = [t.numpy() for t in carve(self._out_host)]
        bos = int(self.cfg.token_nums) - 3
        self._bos = torch.full((1, self.prefix), bos, dtype=torch.int64, device=dev)
        self.image = torch.empty((1, self.n_cams, 3, self.crop, self.crop), dtype=torch.float32,
                                 device=dev)
        self.rgb_crops = (torch.empty((self.n_cams, self.crop, self.crop, 3), dtype=torch.uint8,
                                      device=dev) if self.display else None)
        self.seg_image = None
        self.pred_segmentation = self.target_bev = self.tokens = None
        self._ws = None
        self._graph = None
        self._rig = self._rig_ids = self._rig_versions = None
        self._data = None
        self._use_noise = None
        self.graph_memsets = 0

    # -- the captured chain ---------------------------------------------------------------
    def _run(self):
        decode_bgra(self.frames, self.crop, out_image=self.image[0], out_rgb=self.rgb_crops)
        target_select(self.state, self._goal, out=self.target_point_used)
        with torch.no_grad():
            toks, seg, _, target_bev = self.model.predict(
                self._data, self._noise if self._use_noise else None)
        B, C, X, Y = seg.shape
        if self._ws is None:  # first (eager) run only: nothing is allocated under capture
            self._ws = slot_workspace(B, X, seg.device)
            if self.display:
                self.seg_image = torch.empty((B, X, Y), dtype=torch.uint8, device=seg.device)
        if toks.shape[1] != self.T:
            raise _lib.E2EPError(f"AgentStep: predict returned {toks.shape[1]} tokens, expected "
                                 f"{self.T}")
        slot_stats(seg, self.state, self.res, target_class=2, workspace=self._ws,
                   class_image=self.seg_image, found=self._found, stats=self._stats, seq=toks,
                   first=self.prefix, token_nums=int(self.cfg.token_nums),
                   controls=self._controls, tokens_out=self._tokens)
        self.tokens, self.pred_segmentation, self.target_bev = toks, seg, target_bev
        return toks, seg, target_bev

    def _first_tick(self, intrinsics, extrinsics):
        self._rig = _rig_key(intrinsics, extrinsics)
        self._rig_ids = (intrinsics, extrinsics)
        self._data = {"image": self.image, "target_point": self.target_point_used,
                      "ego_motion": self._ego, "gt_control": self._bos,
                      "intrinsics": intrinsics, "extrinsics": extrinsics}
        if not self.capture:
            return
        # eager warm-up on a side stream (plans the rig, fills every cache the capture reuses),
        # with the state put back so the warm-up is not a tick; then the capture
        keep = self.state.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._run()
            self.state.copy_(keep)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._graph, _, self.graph_memsets = graphs.capture(self._run)

    def _check_rig(self, intrinsics, extrinsics):
        if intrinsics is self._rig_ids[0] and extrinsics is self._rig_ids[1]:
            if self._rig_versions == (intrinsics._version, extrinsics._version):
                return
        if _rig_key(intrinsics, extrinsics) != self._rig:
            raise _lib.E2EPError(
                "AgentStep: this tick's intrinsics/extrinsics differ from the camera rig fixed "
                "at the first tick (the lift-splat plan is part of the step); build a new "
                "AgentStep for a new rig")

    # -- public ---------------------------------------------------------------------------
    def reset(self):
        """Forget the fed-back target point (init_agent's pre_target_point = None)."""
        self.state.zero_()

    def _stage_frames(self, frames):
        if isinstance(frames, (list, tuple)) and frames and hasattr(frames[0], "raw_data"):
            if len(frames) != self.n_cams:
                raise _lib.E2EPError(f"AgentStep: {len(frames)} frames for {self.n_cams} cameras")
            for i, f in enumerate(frames):
                if (int(f.height), int(f.width)) != (self.H, self.W):
                    raise _lib.E2EPError(f"AgentStep: frame {i} is {f.height} x {f.width}, "
                                         f"expected {self.H} x {self.W}")
                a = np.frombuffer(f.raw_data, dtype=np.uint8)
                self._frames_host[i].view(-1).numpy()[:] = a
            return
        t = torch.as_tensor(np.asarray(frames) if not torch.is_tensor(frames) else frames)
        if t.dtype != torch.uint8 or tuple(t.shape) != tuple(self._frames_host.shape):
            raise _lib.E2EPError(f"AgentStep: frames must be uint8 {tuple(self._frames_host.shape)}, "
                                 f"got {t.dtype} {tuple(t.shape)}")
        if t.is_cuda:
            raise _lib.E2EPError("AgentStep: pass the raw frames as host bytes (they are uploaded "
                                 "with the tick's scalars in one copy)")
        self._frames_host.copy_(t)

    def tick(self, frames, ego_motion, goal_target_point, intrinsics, extrinsics, noise=None):
        self._stage_frames(frames)
        sc = self._sc_host
        sc[0:3] = torch.as_tensor(ego_motion, dtype=torch.float32).reshape(3)
        sc[3:6] = torch.as_tensor(goal_target_point, dtype=torch.float32).reshape(3)
        if self._use_noise is None:
            self._use_noise = noise is not None
        elif self._use_noise != (noise is not None):
            raise _lib.E2EPError("AgentStep: `noise` must be passed on every tick or on none (the "
                                 "choice is part of the step fixed at the first tick)")
        if noise is not None:
            sc[6:8] = torch.as_tensor(noise, dtype=torch.float32).reshape(2)
        self._in_dev.copy_(self._in_host, non_blocking=True)
        if self._rig is None:
            self._first_tick(intrinsics, extrinsics)
            self._rig_versions = (intrinsics._version, extrinsics._version)
        else:
            self._check_rig(intrinsics, extrinsics)
        if self._graph is not None:
            self._graph.replay()
        else:
            self._run()
        self._out_host.copy_(self._out_dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        controls, tokens, stats, used, state, found = self._h
        r = TickResult()
        c = controls[0]
        r.controls = [float(c[0]), float(c[1]), float(c[2]), bool(c[3] != 0.0)]
        r.tokens = [int(v) for v in tokens[0]]
        r.target_point_used = [float(v) for v in used[0]]
        r.slot_found = bool(found[0])
        r.slot_stats = tuple(int(v) for v in stats[0])
        r.next_target = [float(state[0, 1]), float(state[0, 2])] if state[0, 0] != 0 else None
        return r
