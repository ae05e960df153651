"""Fused flat Adam for the ParkingModel train step (csrc/adam.hip).

The reference optimises with torch.optim.Adam(lr, weight_decay) over ~570 parameter
tensors (trainer/pl_trainer.py:116-121).  Stepping them tensor by tensor costs thousands
of small launches per step (and accumulating every gradient into a zeroed .grad another
~570).  Here all parameters live in ONE flat fp32 buffer (each nn.Parameter's storage is a
16-byte-aligned view into it), exp_avg / exp_avg_sq are flat buffers of the same layout,
and one launch steps everything, reading each gradient straight from the tensor autograd
produced (a device table of gradient addresses; .grad is set to None before backward so
autograd hands its result over without an accumulate).  For data parallelism the
gradients are gathered into a flat buffer of the same layout by one more launch, and
that buffer is what RCCL all-reduces.

FlatAdam is a torch.optim.Optimizer, so the reference's CosineAnnealingLR
(trainer/pl_trainer.py:120) binds to it unchanged.  The learning rates the kernel uses live
in a device fp64 array `lr_dev`, one value per parameter group: step() (eager) and TrainStep
(before each graph replay) copy every param_groups[k]['lr'] into it when the scheduler has
changed any of them (sync_lr), so a captured step follows the schedule.  betas / eps /
weight_decay are fixed at construction (the reference never changes them).

Parameter groups.  `params` is a parameter list (one group) or a list of torch-style group
dicts with the per-group keys `lr`, `weight_decay` and `decoupled_weight_decay` (torch 2.10's
names; the constructor's arguments are the defaults; `name` and other keys are kept); betas
and eps are shared (a group that overrides them: ValueError).  decoupled_weight_decay is
AdamW's p *= 1 - lr * wd in place of the L2 term g += wd * p.  The chunk table's fourth int
per row is the tensor's group, and `wd_dev` (fp64) / `flags_dev` (int32; bit 0: decoupled),
written at construction and by load_state_dict, hold the other per-group values: still ONE
update launch (e2ep_adam_step_groups), the same 7 x 4 bytes per weight; the gradient norm, the
clip coefficient, the step counter, `stepped` and the average are global.  `order=` (a
sequence of all the parameters; default: the groups concatenated) fixes the flat layout and
with it the meaning of the indices in `params`, `spans`, `chunk_rows`, `group_of` and
ema_param(i): with order= the module's parameter order, TrainStep, the gradient buckets, the
segmented exchange and the checkpoint's "ema" entry see the layout they see without groups.
A parameter in two groups, or an `order` that is not the groups' set of parameters, is a
ValueError, and so is add_param_group (the layout is fixed).  `lr` means group 0.  One group
without decoupled decay takes exactly the calls it always took (e2ep_adam_step, _clipped or
_ema); every other optimizer takes e2ep_adam_step_groups, whose result for groups with equal
hyper-parameters is bit for bit the ungrouped one.
parameter_groups(module, ...) builds the usual fine-tuning recipe: a lower learning rate for
the pretrained cam_encoder.backbone, no decay on norm scales, biases and pos_embed.

state_dict() / load_state_dict() use torch.optim.Adam's format, so checkpoints move
between this optimizer and the reference's: one entry per group, parameter indices in
torch's convention (the groups concatenated), mapped through the layout permutation
(layout_to_torch).  A torch.optim.Adam built with the same groups loads a FlatAdam state and
the other way round.

Optional, all off by default (step() then makes exactly the calls it always made):
  * max_grad_norm: global gradient-norm clipping, torch.nn.utils.clip_grad_norm_'s formula
    (Lightning's gradient_clip_val).  step() becomes three entry-point calls, four kernel
    launches, in one capturable chain: one fp64 sum of squares per chunk-table row
    (k_gnorm_partial), one workgroup that sums them in a fixed order and writes the norm, the
    clip coefficient and a skip flag to device memory (k_gnorm_final), and the step counter and
    Adam launches that read the coefficient and the flag there (k_adam_count_unless,
    k_adam_clip).  No host synchronisation: the norm
    (`grad_norm_dev`, float64, before clipping), `clip_coef_dev` and `skipped_dev` are
    persistent device tensors, and reading them is the caller's synchronisation.  The norm is
    reproducible bit for bit: it does not depend on the gradient source (table or flat
    buffer), on a gradient's alignment, or on eager launch versus graph replay.
  * skip_nonfinite: an update whose gradient norm is Inf or NaN changes nothing (parameters,
    moments, step counter, stepped flags) and is counted in `skipped_dev`.
  * accumulate_grads(flat, first) / has_grad(out, union=True): gradient accumulation into a
    flat buffer over several micro-steps (Lightning's accumulate_grad_batches), followed by
    step(flat, 1 / micro_steps, has_grad=union).
The two settings are attributes and no optimizer state (state_dict() does not carry them); a
captured step keeps the values it was captured with.

Exponential moving average of the weights (ema_decay=, ema_warmup=; off by default, then
nothing is allocated and step() makes the calls it always made).  `ema` is a fourth flat
buffer in the parameter layout, initialised to the parameters; step() calls
e2ep_adam_step_ema in place of either Adam entry point, whose update launch also forms
ema += (1 - d_t) * (p_new - ema) while the new weight is in a register (9 x 4 bytes per weight
instead of 7 x 4, no extra launch).  d_t = ema_decay, or with ema_warmup
min(ema_decay, (1 + n) / (10 + n)) for the n-th update (timm's ModelEmaV2 warm-up); n lives in
`ema_updates_dev` (int64, device), so a captured step warms up under replay.  A tensor without
a gradient keeps its weights and still averages toward them
(torch.optim.swa_utils.AveragedModel.update_parameters); a skipped step changes neither the
average nor the counter.  Under data parallelism every rank computes the same average from
the same weights: nothing is exchanged.
`with opt.ema_weights():` evaluates with the averaged weights: ONE e2ep_flat_swap launch
exchanges the contents of `flat` and `ema` (the live weights are parked in `ema`), the exit
swaps back.  No parameter's address changes, so captured TrainStep / ValStep / AgentStep
graphs see the averaged weights with nothing re-captured.  Swap once per validation epoch,
around the whole loop over batches, not once per batch.  While the context is active the
optimizer refuses to step, accumulate, reset or load the average.
BatchNorm running statistics are module buffers, not parameters, and already moving
averages: they are no part of FlatAdam and are neither averaged nor swapped.
The average is no torch.optim.Adam state: state_dict() / load_state_dict() do not carry it
(ema_state() / load_ema_state() do; checkpoint.py stores it next to the weights).
"""
import contextlib

import torch

from . import _lib

_ALIGN = 4  # elements (16 bytes)


def layout_to_torch(groups):
    """`groups`: per parameter group, the layout positions of its parameters.  Returns `t` with
    t[layout position] = the parameter's index in torch.optim's state_dict() convention (the
    groups concatenated).  Every position 0 .. n-1 must appear exactly once."""
    cat = [i for g in groups for i in g]
    if sorted(cat) != list(range(len(cat))):
        raise ValueError("layout_to_torch: the groups are no partition of 0 .. n-1")
    t = [0] * len(cat)
    for k, i in enumerate(cat):
        t[i] = k
    return t


def parameter_groups(module, lr, weight_decay, backbone_lr_scale=1.0, no_decay_norm_bias=False,
                     decoupled=False):
    """The fine-tuning recipe as parameter groups: -> (groups, order).  `order` is the module's
    trainable parameters in module order (FlatAdam's order=, so TrainStep and the exchange see
    the layout they see without groups).  The groups are the non-empty cells of
      backbone (name contains `cam_encoder.backbone.`, lr * backbone_lr_scale) / rest, taken
        only when backbone_lr_scale != 1;
      decay / no_decay (p.ndim <= 1: norm scales and biases, or a name ending in `pos_embed`;
        weight_decay 0), taken only with no_decay_norm_bias;
    named backbone_decay, backbone_no_decay, rest_decay, rest_no_decay, each a dict
    {"params", "lr", "weight_decay", "decoupled_weight_decay", "name"} that torch.optim.Adam
    and FlatAdam both take.  With the default arguments there is one group (rest_decay: every
    trainable parameter): build the plain one-group optimizer from `order` then."""
    named = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
    order = [p for _, p in named]
    split_bb = float(backbone_lr_scale) != 1.0
    cells = {}
    for n, p in named:
        bb = split_bb and "cam_encoder.backbone." in n
        nd = bool(no_decay_norm_bias) and (p.ndim <= 1 or n.endswith("pos_embed"))
        cells.setdefault((bb, nd), []).append(p)
    groups = []
    for bb in (True, False):
        for nd in (False, True):
            if (bb, nd) in cells:
                groups.append({"params": cells[(bb, nd)],
                               "lr": lr * backbone_lr_scale if bb else lr,
                               "weight_decay": 0.0 if nd else weight_decay,
                               "decoupled_weight_decay": bool(decoupled),
                               "name": ("backbone" if bb else "rest") + ("_no_decay" if nd else "_decay")})
    return groups, order


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False,
                 decoupled_weight_decay=False, order=None):
        params = list(params)
        if not params:
            raise ValueError("FlatAdam: empty parameter list")
        self._layout_fixed = False
        if isinstance(params[0], dict):
            groups = [dict(g, params=list(g["params"])) for g in params]
            for g in groups:
                if tuple(g.get("betas", betas)) != tuple(betas) or g.get("eps", eps) != eps:
                    raise ValueError("FlatAdam: betas and eps are shared by all parameter groups")
        else:
            groups = [{"params": params}]
        cat = [p for g in groups for p in g["params"]]
        if not cat:
            raise ValueError("FlatAdam: empty parameter list")
        if len({id(p) for p in cat}) != len(cat):
            raise ValueError("FlatAdam: a parameter appears in more than one parameter group")
        if order is not None:
            order = list(order)
            if len(order) != len(cat) or {id(p) for p in order} != {id(p) for p in cat}:
                raise ValueError("FlatAdam: `order` and the parameter groups do not hold the "
                                 "same parameters")
        dev = cat[0].device
        if dev.type != "cuda":
            raise _lib.E2EPError("FlatAdam runs on a HIP device only")
        for p in cat:
            if p.dtype != torch.float32 or p.device != dev:
                raise _lib.E2EPError("FlatAdam: parameters must be fp32 on one device")
        super().__init__(groups, dict(lr=lr, betas=tuple(betas), eps=eps,
                                      weight_decay=weight_decay,
                                      decoupled_weight_decay=bool(decoupled_weight_decay)))
        self._layout_fixed = True
        # the flat layout: `order`, else the groups concatenated (one group: its own list)
        self.params = (order if order is not None else
                       self.param_groups[0]["params"] if len(groups) == 1 else cat)
        pos = {id(p): i for i, p in enumerate(self.params)}
        layout = [[pos[id(p)] for p in g["params"]] for g in self.param_groups]
        self._torch_index = layout_to_torch(layout)
        gid = [0] * len(self.params)
        for k, g in enumerate(layout):
            for i in g:
                gid[i] = k
        self.group_of = gid  # layout position -> parameter group
        self.betas, self.eps = tuple(betas), eps
        self.weight_decay = self.param_groups[0]["weight_decay"]
        lib = _lib.load()
        chunk = lib.e2ep_adam_chunk_elems()
        offs, rows, off = [], [], 0
        for i, p in enumerate(self.params):
            offs.append(off)
            n = p.numel()
            for s in range(0, n, chunk):
                rows.append((i, s, min(chunk, n - s), gid[i]))
            off += (n + _ALIGN - 1) // _ALIGN * _ALIGN
        self.numel = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(self.params, offs):
                v = self.flat[o:o + p.numel()].view_as(p)
                v.copy_(p)
                p.data = v
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.step_count = torch.zeros(1, dtype=torch.float32, device=dev)
        # 1 for every tensor stepped at least once (written by the Adam kernel): state_dict
        # holds state for those only, as torch.optim.Adam does (a tensor that never had a
        # gradient, e.g. bev_encoder.layer4, has no state there)
        self.stepped = torch.zeros(len(self.params), dtype=torch.int32, device=dev)
        self.offsets = torch.tensor(offs, dtype=torch.int64, device=dev)
        self.chunks = torch.tensor(rows, dtype=torch.int32, device=dev).reshape(-1)
        self.n_chunks = len(rows)
        self._offs_host = offs
        self.spans = [(o, p.numel()) for o, p in zip(offs, self.params)]
        self._gtab = torch.zeros(len(self.params), dtype=torch.int64, device=dev)
        self._has_bool = torch.zeros(len(self.params), dtype=torch.bool, device=dev)
        self._gkey = None
        # row range of each tensor in the chunk table (gradient buckets gather by rows)
        self.chunk_rows, r = [], 0
        for p in self.params:
            n = (p.numel() + chunk - 1) // chunk
            self.chunk_rows.append((r, r + n))
            r += n
        # one learning rate, weight decay and flag word (bit 0: decoupled) per group, in device
        # memory: the grouped launch indexes them by the chunk row's group
        lrs = [float(g["lr"]) for g in self.param_groups]
        self.n_groups = len(lrs)
        self.lr_dev = torch.tensor(lrs, dtype=torch.float64, device=dev)
        self._lr_written = lrs
        self.wd_dev = torch.zeros(self.n_groups, dtype=torch.float64, device=dev)
        self.flags_dev = torch.zeros(self.n_groups, dtype=torch.int32, device=dev)
        self._write_group_tables()
        # gradient-norm clipping / non-finite skip (module docstring): settings, the device
        # scalars the chain writes, and its workspace (one fp64 partial per chunk-table row)
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self.grad_norm_dev = torch.zeros(1, dtype=torch.float64, device=dev)
        self.clip_coef_dev = torch.ones(1, dtype=torch.float32, device=dev)
        self.skipped_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._skip_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._partials = torch.zeros(self.n_chunks, dtype=torch.float64, device=dev)
        self._has_i64 = torch.zeros(len(self.params), dtype=torch.int64, device=dev)
        # weight averaging (module docstring): nothing is allocated while it is off
        self.ema_decay, self.ema_warmup = None, False
        self.ema = self.ema_updates_dev = None
        self._ema_swapped = False
        if ema_decay is not None:
            self.enable_ema(ema_decay, ema_warmup)

    # -- weight averaging ---------------------------------------------------------------------
    def enable_ema(self, decay, warmup=False):
        """Switch weight averaging on (or change its settings): 0 <= decay < 1.  The first call
        allocates `ema` as a copy of the parameters and the update counter at 0; a later one
        keeps both.  Outside graph capture and before the step is captured."""
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"FlatAdam: ema_decay must be in [0, 1), got {decay}")
        self._ema_guard("enable_ema")
        self.ema_decay, self.ema_warmup = decay, bool(warmup)
        if self.ema is None:
            self.ema = torch.empty_like(self.flat).copy_(self.flat)  # pads are zero, as flat's
            self.ema_updates_dev = torch.zeros(1, dtype=torch.int64, device=self.flat.device)

    def _ema_guard(self, what, need_ema=False):
        if need_ema and self.ema is None:
            raise _lib.E2EPError(f"FlatAdam.{what}: weight averaging is off (ema_decay=None)")
        if self._ema_swapped:
            raise _lib.E2EPError(f"FlatAdam.{what} inside ema_weights(): the parameters hold "
                                 "the averaged weights")
        if torch.cuda.is_current_stream_capturing():
            raise _lib.E2EPError(f"FlatAdam.{what} during stream capture")

    def ema_param(self, i):
        """The averaged values of parameter i (a view of `ema` shaped like it).  Inside
        ema_weights() the buffers are exchanged: this is then the parked live parameter."""
        if self.ema is None:
            raise _lib.E2EPError("FlatAdam.ema_param: weight averaging is off (ema_decay=None)")
        o, n = self.spans[i]
        return self.ema[o:o + n].view_as(self.params[i])

    def reset_ema(self):
        """ema = the current parameters, update counter = 0.  Not during capture."""
        self._ema_guard("reset_ema", need_ema=True)
        self.ema.copy_(self.flat)
        self.ema_updates_dev.zero_()

    def ema_state(self):
        """{"decay", "warmup", "num_updates", "flat": a clone of `ema`} (reading the counter
        synchronises)."""
        self._ema_guard("ema_state", need_ema=True)
        return {"decay": float(self.ema_decay), "warmup": bool(self.ema_warmup),
                "num_updates": int(self.ema_updates_dev.item()), "flat": self.ema.clone()}

    def load_ema_state(self, state):
        """Load what ema_state() returned (settings, counter and the averaged weights)."""
        self._ema_guard("load_ema_state", need_ema=True)
        flat = state["flat"]
        if flat.numel() != self.numel:
            raise ValueError(f"FlatAdam.load_ema_state: {flat.numel()} values for a layout of "
                             f"{self.numel}")
        decay = float(state["decay"])
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"FlatAdam: ema_decay must be in [0, 1), got {decay}")
        self.ema_decay, self.ema_warmup = decay, bool(state["warmup"])
        self.ema.copy_(flat.reshape(-1))
        self.ema_updates_dev.fill_(int(state["num_updates"]))

    def _swap(self):
        _lib.call("e2ep_flat_swap", _lib.ptr(self.flat), _lib.ptr(self.ema), self.numel,
                  _lib.stream())

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate with the averaged weights: one launch exchanges the contents of `flat` and
        `ema` on entry and one exchanges them back on exit, on the current stream (module
        docstring).  Does not nest; not during stream capture."""
        self._ema_guard("ema_weights", need_ema=True)
        self._swap()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._swap()
            self._ema_swapped = False

    @property
    def ema_active(self):
        """True inside ema_weights()."""
        return self._ema_swapped

    # -- learning rate ------------------------------------------------------------------------
    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, v):
        self.param_groups[0]["lr"] = v

    def sync_lr(self):
        """Copy every group's param_groups[k]['lr'] (an LR scheduler's output) into the device
        array the Adam kernel reads, if any of them changed.  Not during capture: the kernel
        node reads the array at replay time, the host writes it between replays."""
        lrs = [float(g["lr"]) for g in self.param_groups]
        if lrs != self._lr_written and not torch.cuda.is_current_stream_capturing():
            if len(lrs) == 1:
                self.lr_dev.fill_(lrs[0])
            else:
                self.lr_dev.copy_(torch.tensor(lrs, dtype=torch.float64))
            self._lr_written = lrs

    # -- parameter groups ---------------------------------------------------------------------
    def add_param_group(self, param_group):
        if self._layout_fixed:
            raise ValueError("FlatAdam: the flat layout is fixed at construction; parameter "
                             "groups cannot be added afterwards")
        super().add_param_group(param_group)

    def _write_group_tables(self):
        """param_groups' weight_decay / decoupled_weight_decay -> wd_dev / flags_dev (at
        construction and after load_state_dict; the learning rates go through sync_lr), and
        which entry point step() takes: one L2 group keeps the three ungrouped ones."""
        wds = [float(g["weight_decay"]) for g in self.param_groups]
        dec = [bool(g.get("decoupled_weight_decay", False)) for g in self.param_groups]
        self.wd_dev.copy_(torch.tensor(wds, dtype=torch.float64))
        self.flags_dev.copy_(torch.tensor([int(d) for d in dec], dtype=torch.int32))
        self.weight_decay = self.param_groups[0]["weight_decay"]
        self.grouped = len(wds) > 1 or dec[0]

    # -- gradients --------------------------------------------------------------------------
    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    def prepare(self, params=None):
        """Point the device gradient table at the current .grad tensors (one small H2D copy,
        only when an address changed) — of all tensors, or of the index range `params` =
        (i0, i1) (one gradient bucket).  Call it outside graph capture."""
        i0, i1 = params if params is not None else (0, len(self.params))
        key = []
        for p in self.params[i0:i1]:
            g = p.grad
            if g is None:
                key.append(0)
                continue
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.flat.device:
                raise _lib.E2EPError("FlatAdam: gradients must be contiguous fp32 on the device")
            key.append(g.data_ptr())
        old = self._gkey if self._gkey is not None else (None,) * len(self.params)
        if tuple(key) != tuple(old[i0:i1]):
            if torch.cuda.is_current_stream_capturing():
                raise _lib.E2EPError("FlatAdam.prepare: gradient addresses changed during capture")
            self._gtab[i0:i1].copy_(torch.tensor(key, dtype=torch.int64))
            self._gkey = tuple(old[:i0]) + tuple(key) + tuple(old[i1:])

    def gather_grads(self, out, params=None):
        """Per-tensor gradients -> `out` (flat, parameter layout) for the all-reduce;
        `params` = (i0, i1) restricts it to one bucket of tensors."""
        if params is None:
            r0, r1 = 0, self.n_chunks
        else:
            r0, r1 = self.chunk_rows[params[0]][0], self.chunk_rows[params[1] - 1][1]
        if r1 <= r0:
            return
        import ctypes
        _lib.call("e2ep_grad_gather", ctypes.c_void_p(self.chunks.data_ptr() + 16 * r0), r1 - r0,
                  _lib.ptr(self.offsets), _lib.ptr(self._gtab), _lib.ptr(out), _lib.stream())

    def accumulate_grads(self, flat, first):
        """One micro-step of gradient accumulation into `flat` (parameter layout), from the
        prepared table: the first micro-step of a cycle gathers (zeros for a tensor without a
        gradient, so `flat` needs no clearing), every later one adds (such a tensor adds
        nothing).  Pair it with has_grad(out, union=not first), then
        step(flat, 1 / micro_steps, has_grad=out)."""
        if self._ema_swapped:
            self._ema_guard("accumulate_grads")
        if first:
            self.gather_grads(flat)
            return
        _lib.call("e2ep_grad_accumulate", _lib.ptr(self.chunks), self.n_chunks,
                  _lib.ptr(self.offsets), _lib.ptr(self._gtab), _lib.ptr(flat), _lib.stream())

    # -- update -----------------------------------------------------------------------------
    @torch.no_grad()
    def has_grad(self, out, union=False):
        """out[i] = 1 if parameter i has a gradient this step (from the prepared table), else 0
        (int64, capturable).  Data-parallel callers all-reduce it with MAX and pass it to
        step(grad_flat, ..., has_grad=out): every replica then steps the same parameters.
        union=True keeps the entries `out` already has (out[i] = max(out[i], this step's)): over
        an accumulation cycle a parameter with a gradient in any micro-step is stepped, one
        with none in the whole cycle is not."""
        torch.ne(self._gtab, 0, out=self._has_bool)
        if union:
            self._has_i64.copy_(self._has_bool)
            torch.maximum(out, self._has_i64, out=out)
        else:
            out.copy_(self._has_bool)
        return out

    def step(self, grad_flat=None, grad_scale=1.0, closure=None, has_grad=None):
        """One Adam step from the prepared gradient table, or from `grad_flat` (scaled by
        grad_scale, e.g. 1/world for an all-reduced sum); tensors whose table entry is null
        (no gradient) are skipped either way.  With `grad_flat`, `has_grad` (int64 per
        parameter, non-zero = step it; see has_grad()) replaces this rank's own table, so a
        parameter that had a gradient on any rank is stepped on every rank, as under DDP.
        torch.optim-style calls (no arguments, or a closure) prepare the table themselves.
        With max_grad_norm or skip_nonfinite set, the norm of the scaled gradient is taken
        first and the update reads the clip coefficient and the skip flag from device memory
        (module docstring); the norm is over the tensors that are stepped."""
        if self._ema_swapped:
            self._ema_guard("step")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not torch.cuda.is_current_stream_capturing():
            self.prepare()
        self.sync_lr()
        b1, b2 = self.betas
        table = _lib.ptr(has_grad if (has_grad is not None and grad_flat is not None)
                         else self._gtab)
        gflat = _lib.ptr(grad_flat) if grad_flat is not None else None
        plain = self.max_grad_norm is None and not self.skip_nonfinite
        if plain and self.grouped:
            self._step_groups(table, gflat, grad_scale, None, None)
            return loss
        if plain and self.ema is not None:
            self._step_ema(table, gflat, grad_scale, None, None)
            return loss
        if plain:
            _lib.call("e2ep_adam_step", _lib.ptr(self.chunks), self.n_chunks,
                      _lib.ptr(self.offsets), table, gflat,
                      _lib.ptr(self.flat), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                      _lib.ptr(self.step_count), _lib.ptr(self.lr_dev), float(b1), float(b2),
                      float(self.eps), float(self.weight_decay), float(grad_scale),
                      _lib.ptr(self.stepped), _lib.stream())
            return loss
        max_norm = -1.0  # the finalisation's "clipping off": the coefficient is exactly 1
        if self.max_grad_norm is not None:
            max_norm = float(self.max_grad_norm)
            if not max_norm >= 0.0:
                raise ValueError(f"FlatAdam: max_grad_norm must be >= 0, got {self.max_grad_norm}")
        _lib.call("e2ep_grad_sqnorm", _lib.ptr(self.chunks), self.n_chunks, _lib.ptr(self.offsets),
                  table, gflat, _lib.ptr(self._partials), _lib.stream())
        _lib.call("e2ep_grad_norm_finalize", _lib.ptr(self._partials), self.n_chunks,
                  float(grad_scale), max_norm, int(self.skip_nonfinite),
                  _lib.ptr(self.grad_norm_dev), _lib.ptr(self.clip_coef_dev),
                  _lib.ptr(self._skip_dev), _lib.ptr(self.skipped_dev), _lib.stream())
        if self.grouped:
            self._step_groups(table, gflat, grad_scale, self.clip_coef_dev, self._skip_dev)
            return loss
        if self.ema is not None:
            self._step_ema(table, gflat, grad_scale, self.clip_coef_dev, self._skip_dev)
            return loss
        _lib.call("e2ep_adam_step_clipped", _lib.ptr(self.chunks), self.n_chunks,
                  _lib.ptr(self.offsets), table, gflat,
                  _lib.ptr(self.flat), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                  _lib.ptr(self.step_count), _lib.ptr(self.lr_dev), float(b1), float(b2),
                  float(self.eps), float(self.weight_decay), float(grad_scale),
                  _lib.ptr(self.clip_coef_dev), _lib.ptr(self._skip_dev),
                  _lib.ptr(self.stepped), _lib.stream())
        return loss

    def _step_ema(self, table, gflat, grad_scale, coef, skip):
        b1, b2 = self.betas
        _lib.call("e2ep_adam_step_ema", _lib.ptr(self.chunks), self.n_chunks,
                  _lib.ptr(self.offsets), table, gflat,
                  _lib.ptr(self.flat), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                  _lib.ptr(self.step_count), _lib.ptr(self.lr_dev), float(b1), float(b2),
                  float(self.eps), float(self.weight_decay), float(grad_scale),
                  _lib.ptr(coef), _lib.ptr(skip), _lib.ptr(self.stepped),
                  _lib.ptr(self.ema), _lib.ptr(self.ema_updates_dev), float(self.ema_decay),
                  int(self.ema_warmup), _lib.stream())

    def _step_groups(self, table, gflat, grad_scale, coef, skip):
        """The grouped update: clipping (coef, skip) and the average are each on or null."""
        b1, b2 = self.betas
        ema = self.ema is not None
        _lib.call("e2ep_adam_step_groups", _lib.ptr(self.chunks), self.n_chunks,
                  _lib.ptr(self.offsets), table, gflat,
                  _lib.ptr(self.flat), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                  _lib.ptr(self.step_count), _lib.ptr(self.lr_dev), _lib.ptr(self.wd_dev),
                  _lib.ptr(self.flags_dev), self.n_groups, float(b1), float(b2),
                  float(self.eps), float(grad_scale), _lib.ptr(coef), _lib.ptr(skip),
                  _lib.ptr(self.stepped), _lib.ptr(self.ema), _lib.ptr(self.ema_updates_dev),
                  float(self.ema_decay) if ema else 0.0, int(self.ema_warmup) if ema else 0,
                  _lib.stream())

    # -- torch.optim.Adam-format state --------------------------------------------------------
    def state_dict(self):
        """torch.optim.Adam's format: one entry per group, parameter indices in torch's
        convention (the groups concatenated; layout_to_torch maps the layout positions).  One L2
        group gives exactly the dict it always gave; otherwise every group also carries
        `decoupled_weight_decay` (torch's key) and its `name` when it has one."""
        state = {}
        stepped = self.stepped.cpu().tolist()
        for i, (p, o) in enumerate(zip(self.params, self._offs_host)):
            if not stepped[i]:
                continue
            n = p.numel()
            state[self._torch_index[i]] = {
                "step": self.step_count[0].detach().cpu().clone(),
                "exp_avg": self.exp_avg[o:o + n].view_as(p).clone(),
                "exp_avg_sq": self.exp_avg_sq[o:o + n].view_as(p).clone()}
        state = {k: state[k] for k in sorted(state)}
        groups, first = [], 0
        for g in self.param_groups:
            n = len(g["params"])
            group = {"lr": float(g["lr"]), "betas": self.betas, "eps": self.eps,
                     "weight_decay": g["weight_decay"], "amsgrad": False, "maximize": False,
                     "foreach": None, "capturable": False, "differentiable": False, "fused": None}
            if self.grouped:
                group["decoupled_weight_decay"] = bool(g.get("decoupled_weight_decay", False))
                if "name" in g:
                    group["name"] = g["name"]
            if "initial_lr" in g and self.grouped:
                group["initial_lr"] = g["initial_lr"]
            group["params"] = list(range(first, first + n))
            groups.append(group)
            first += n
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        saved = sd["param_groups"]
        if len(saved) != len(self.param_groups) or any(
                len(g["params"]) != len(pg["params"]) for g, pg in zip(saved, self.param_groups)):
            raise ValueError("FlatAdam.load_state_dict: the state's parameter groups do not "
                             "match the optimizer's")
        if any(tuple(g["betas"]) != tuple(saved[0]["betas"]) or g["eps"] != saved[0]["eps"]
               for g in saved):
            raise ValueError("FlatAdam: betas and eps are shared by all parameter groups")
        self.betas, self.eps = tuple(saved[0]["betas"]), saved[0]["eps"]
        for g, pg in zip(saved, self.param_groups):
            pg.update(lr=g["lr"], betas=self.betas, eps=self.eps, weight_decay=g["weight_decay"],
                      decoupled_weight_decay=bool(g.get("decoupled_weight_decay", False)))
            if "initial_lr" in g:
                pg["initial_lr"] = g["initial_lr"]
        self._write_group_tables()
        steps = set()
        with torch.no_grad():
            self.stepped.zero_()
            for i, (p, o) in enumerate(zip(self.params, self._offs_host)):
                s = sd["state"].get(self._torch_index[i])
                if s is None:
                    continue
                self.stepped[i] = 1
                n = p.numel()
                self.exp_avg[o:o + n].copy_(s["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + n].copy_(s["exp_avg_sq"].reshape(-1))
                steps.add(float(s["step"]))
        if len(steps) > 1:
            raise ValueError("FlatAdam keeps one step count; the state has several")
        self.step_count.fill_(steps.pop() if steps else 0.0)
