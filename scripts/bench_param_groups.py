"""Cost of FlatAdam's parameter groups (optim.py, csrc/adam.hip: k_adam_groups).

ONE process, two parts, every setting timed in alternating blocks so clock and thermal drift hit
them alike; per setting the median over blocks and their spread (min, max).

A. FlatAdam.step over the full ParkingTrainingModule parameter set (the tensors' names and
   shapes, layer4 frozen as in bench.py; random values, one shared set of gradient tensors):

       one        one group, e2ep_adam_step: the yardstick (the code of the parent commit)
       one2       the same optimizer again: two series of ONE setting, the run-to-run spread
       g4         optim.parameter_groups(backbone_lr_scale=0.1, no_decay_norm_bias=True): four
                  groups, L2 weight decay, e2ep_adam_step_groups
       g4d        the same four groups with decoupled weight decay
       *_ce       each of one / g4 / g4d with clipping, skip and the average on
                  (sqnorm + finalize + e2ep_adam_step_ema or e2ep_adam_step_groups)

   each eager (FlatAdam.step as a host call) and as a replayed graph of the same call (device
   time of the launches).  A block is `--iters` calls, synchronised once at its end; its figure
   is ms per call.  Both paths move 7 x 4 bytes per weight (10 x 4 with clipping and the
   average): `model_bytes` is that times the flat buffer's length, `gbps` model bytes over the
   median replayed time.  `inside_spread` says whether a grouped median lies within the band
   [min, max] of the blocks of both one-group series.

B. The captured C2 train step (ParkingModel, B = 8, 4 x 256^2, fp32; bench.py's workload) with
   the config keys off (one group) and on (four groups, decoupled), and the off step a second
   time.

    python scripts/bench_param_groups.py [--iters 200] [--blocks 9] [--step-block 10] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "e2e-parking-carla_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

CE = dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.999, ema_warmup=True)
RECIPE = dict(backbone_lr_scale=0.1, no_decay_norm_bias=True)
SETTINGS = {"one": (None, {}), "g4": (False, {}), "g4d": (True, {}),
            "one_ce": (None, CE), "g4_ce": (False, CE), "g4d_ce": (True, CE)}


def _stats(t):
    t = np.asarray(t)
    return {"median_ms": round(float(np.median(t)), 5), "min_ms": round(float(t.min()), 5),
            "max_ms": round(float(t.max()), 5), "blocks_ms": [round(float(x), 5) for x in t]}


def _alternate(fns, blocks):
    """fns: name -> callable returning one block's ms per call.  One warm-up block each, then
    `blocks` rounds, rotating who goes first."""
    order = list(fns)
    for n in order:
        fns[n]()
    times = {n: [] for n in order}
    for r in range(blocks):
        k = r % len(order)
        for n in order[k:] + order[:k]:
            times[n].append(fns[n]())
    return {n: _stats(t) for n, t in times.items()}


def _block(call, iters):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3
    return run


def _module(dev, **cfg):
    from tool.config import default_cfg
    from trainer.pl_trainer import ParkingTrainingModule
    torch.manual_seed(1234)
    mod = ParkingTrainingModule(default_cfg(**cfg)).to(dev).train()
    for p in mod.parking_model.bev_encoder.layer4.parameters():
        p.requires_grad_(False)
    return mod


class _Named:
    """What optim.parameter_groups reads of a module: named_parameters()."""

    def __init__(self, named):
        self.named = named

    def named_parameters(self):
        return iter(self.named)


def _compare(res, base, base2):
    lo = min(res[base]["min_ms"], res[base2]["min_ms"])
    hi = max(res[base]["max_ms"], res[base2]["max_ms"])
    for n, r in res.items():
        if n not in (base, base2):
            r["over_" + base] = round(r["median_ms"] / res[base]["median_ms"], 4)
            if n.endswith("_ce") == base.endswith("_ce"):
                r["inside_spread"] = bool(lo <= r["median_ms"] <= hi)
    return {"min_ms": lo, "max_ms": hi,
            "median_gap_ms": round(abs(res[base]["median_ms"] - res[base2]["median_ms"]), 5)}


def bench_optimizer(a, dev):
    from e2ep_amd import graphs
    from e2ep_amd.optim import FlatAdam, parameter_groups
    spec = [(n, tuple(p.shape)) for n, p in _module(dev).named_parameters() if p.requires_grad]
    g = torch.Generator(device=dev).manual_seed(0)
    grads = [torch.randn(s, generator=g, device=dev) * 1e-3 for _, s in spec]
    opts = {}
    for name, (decoupled, kw) in SETTINGS.items():
        named = [(n, torch.nn.Parameter(torch.randn(s, generator=g, device=dev) * 0.02)) for n, s in spec]
        ps = [p for _, p in named]
        if decoupled is None:
            opts[name] = FlatAdam(ps, lr=1e-4, weight_decay=1e-4, **kw)
        else:
            groups, order = parameter_groups(_Named(named), 1e-4, 1e-4, decoupled=decoupled, **RECIPE)
            opts[name] = FlatAdam(groups, lr=1e-4, weight_decay=1e-4, order=order,
                                  decoupled_weight_decay=decoupled, **kw)
        for p, gr in zip(ps, grads):
            p.grad = gr  # read-only: every optimizer reads the same gradient tensors
        opts[name].step()
    torch.cuda.synchronize()
    g4 = opts["g4"]
    res = {"tensors": len(spec), "weights": int(sum(int(np.prod(s)) for _, s in spec)),
           "flat_elems": int(g4.numel), "chunk_rows": int(g4.n_chunks),
           "groups": [{"name": pg["name"], "tensors": len(pg["params"]),
                       "weights": int(sum(p.numel() for p in pg["params"])), "lr": pg["lr"],
                       "weight_decay": pg["weight_decay"]} for pg in g4.param_groups],
           "iters_per_block": a.iters, "blocks": a.blocks}
    eager = {n: _block(o.step, a.iters) for n, o in opts.items()}
    eager["one2"], eager["one_ce2"] = eager["one"], eager["one_ce"]
    res["eager"] = _alternate(eager, a.blocks)
    replay = {}
    for n, o in opts.items():
        gr, _, _ = graphs.capture(o.step)
        replay[n] = _block(gr.replay, a.iters)
    replay["one2"], replay["one_ce2"] = replay["one"], replay["one_ce"]
    res["replay"] = _alternate(replay, a.blocks)
    for n, r in res["replay"].items():
        r["model_bytes"] = (10 if "_ce" in n else 7) * 4 * res["flat_elems"]
        r["gbps"] = round(r["model_bytes"] / (r["median_ms"] * 1e-3) / 1e9, 1)
    for kind in ("eager", "replay"):
        plain = {n: r for n, r in res[kind].items() if "_ce" not in n}
        ce = {n: r for n, r in res[kind].items() if "_ce" in n}
        res[kind + "_spread"] = {"one": _compare(plain, "one", "one2"),
                                 "one_ce": _compare(ce, "one_ce", "one_ce2")}
    return res


def bench_train_step(a, dev):
    from e2ep_amd import synthetic
    from e2ep_amd.train import TrainStep
    host = synthetic.synthetic_batch(a.batch, seed=0)
    steps = {}
    for n, cfg in (("off", {}), ("groups", dict(decoupled_weight_decay=True, **RECIPE))):
        mod = _module(dev, **cfg)
        data = {k: (v if k in ("intrinsics", "extrinsics") else v.to(dev)) for k, v in host.items()}
        steps[n] = TrainStep(mod, data, lr=mod.cfg.learning_rate, weight_decay=mod.cfg.weight_decay,
                             graph=True, warmup=2)
    assert not steps["off"].opt.grouped and steps["groups"].opt.n_groups == 4
    fns = {n: _block(s, a.step_block) for n, s in steps.items()}
    fns["off2"] = fns["off"]
    res = _alternate(fns, a.step_blocks)
    for n in list(res):
        if n != "off":
            res[n]["minus_off_ms"] = round(res[n]["median_ms"] - res["off"]["median_ms"], 4)
    res["off_spread_ms"] = round(res["off"]["max_ms"] - res["off"]["min_ms"], 4)
    res["config"] = (f"TrainStep (fwd + 3 losses + bwd + Adam), B={a.batch}, 4x256^2, fp32, captured; "
                     f"ms per call, {a.step_block} calls per block")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="optimizer calls per block")
    ap.add_argument("--blocks", type=int, default=9, help="timed blocks per optimizer setting")
    ap.add_argument("--step-block", type=int, default=10, help="train-step calls per block")
    ap.add_argument("--step-blocks", type=int, default=12, help="timed blocks per train step")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from e2ep_amd import _lib
    _lib.load()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0)}
    res["optimizer"] = bench_optimizer(a, dev)
    if not a.no_train_step:
        res["train_step"] = bench_train_step(a, dev)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
