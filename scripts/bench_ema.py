"""Cost of FlatAdam's exponential moving average of the weights (optim.py, csrc/adam.hip).

ONE process, two parts, every setting timed in alternating blocks so clock and thermal drift hit
them alike; per setting the median over blocks and their spread (min, max).

A. FlatAdam.step over the full ParkingTrainingModule parameter set (the tensors' shapes, layer4
   frozen as in bench.py; random values, one shared set of gradient tensors):

       off        e2ep_adam_step                       7 x 4 bytes per weight
       ema        e2ep_adam_step_ema                   9 x 4
       clip       sqnorm + finalize + adam_step_clipped   (7 + 1) x 4
       ema_clip   sqnorm + finalize + adam_step_ema       (9 + 1) x 4
       off2       the off optimizer again: two series of ONE setting next to the differences
       off_lerp   (replayed only) the off step followed by torch's lerp_ of a separate buffer
                  toward the parameters: the average as a second, 3-access pass  (7 + 3) x 4

   each eager (FlatAdam.step as a host call: the gradient-table check over ~570 tensors and the
   launches) and as a replayed graph of the same call (device time of the launches), plus
   e2ep_flat_swap of the parameter buffer with the average (4 x 4 bytes per weight; plain
   launches back to back, an even number per block, in the replayed series).  A block is
   `--iters` calls, synchronised once at its end; its figure is ms per call.  `model_bytes` is the
   byte model above times the flat buffer's length; `gbps` is model bytes over the median
   replayed time (the count launch and, with clipping, the two norm launches are inside it).

B. The captured C2 train step (ParkingModel, B = 8, 4 x 256^2, fp32; bench.py's workload) with
   the average off and on (decay 0.999, warm-up on), and the off step a second time.

--baseline times the off / clip / off2 settings only and uses nothing this feature added, so the
same file runs on a checkout of the parent commit: the "off" baseline of the comparison.

    python scripts/bench_ema.py [--iters 200] [--blocks 9] [--step-block 10] [--json out.json]
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

ACCESSES = {"off": 7, "off2": 7, "ema": 9, "clip": 8, "ema_clip": 10, "swap": 4, "off_lerp": 10}
OPT = {"off": {}, "ema": dict(ema_decay=0.999, ema_warmup=True),
       "clip": dict(max_grad_norm=1.0, skip_nonfinite=True),
       "ema_clip": dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.999, ema_warmup=True)}


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


def _module(dev):
    from tool.config import default_cfg
    from trainer.pl_trainer import ParkingTrainingModule
    torch.manual_seed(1234)
    mod = ParkingTrainingModule(default_cfg()).to(dev).train()
    for p in mod.parking_model.bev_encoder.layer4.parameters():
        p.requires_grad_(False)
    return mod


def bench_optimizer(a, dev, names):
    from e2ep_amd import _lib, graphs
    from e2ep_amd.optim import FlatAdam
    shapes = [tuple(p.shape) for p in _module(dev).parameters() if p.requires_grad]
    g = torch.Generator(device=dev).manual_seed(0)
    grads = [torch.randn(s, generator=g, device=dev) * 1e-3 for s in shapes]
    opts = {}
    for n in names:
        ps = [torch.nn.Parameter(torch.randn(s, generator=g, device=dev) * 0.02) for s in shapes]
        opts[n] = FlatAdam(ps, lr=1e-4, weight_decay=1e-4, **OPT[n])
        for p, gr in zip(ps, grads):
            p.grad = gr  # read-only: every optimizer reads the same gradient tensors
        opts[n].step()
    torch.cuda.synchronize()
    res = {"tensors": len(shapes), "weights": int(sum(int(np.prod(s)) for s in shapes)),
           "flat_elems": int(opts[names[0]].numel), "iters_per_block": a.iters, "blocks": a.blocks}
    eager = {n: _block(o.step, a.iters) for n, o in opts.items()}
    eager["off2"] = eager["off"]
    res["eager"] = _alternate(eager, a.blocks)
    replay = {}
    for n, o in opts.items():
        gr, _, _ = graphs.capture(o.step)
        replay[n] = _block(gr.replay, a.iters)
    replay["off2"] = replay["off"]
    if "ema" in opts:
        o, shadow = opts["off"], opts["off"].flat.clone()

        def step_then_lerp():
            o.step()
            shadow.lerp_(o.flat, 1e-3)
        gr, _, _ = graphs.capture(step_then_lerp)
        replay["off_lerp"] = _block(gr.replay, a.iters)
        o = opts["ema"]
        replay["swap"] = _block(lambda: _lib.call("e2ep_flat_swap", _lib.ptr(o.flat), _lib.ptr(o.ema),
                                                  o.numel, _lib.stream()), a.iters - a.iters % 2)
    res["replay"] = _alternate(replay, a.blocks)
    for n, r in res["replay"].items():
        r["model_bytes"] = ACCESSES[n] * 4 * res["flat_elems"]
        r["gbps"] = round(r["model_bytes"] / (r["median_ms"] * 1e-3) / 1e9, 1)
    for kind in ("eager", "replay"):
        off = res[kind]["off"]["median_ms"]
        for n in res[kind]:
            if n != "off":
                res[kind][n]["over_off"] = round(res[kind][n]["median_ms"] / off, 4)
    return res


def bench_train_step(a, dev, names):
    from e2ep_amd import synthetic
    from e2ep_amd.train import TrainStep
    host = synthetic.synthetic_batch(a.batch, seed=0)
    steps = {}
    for n in names:
        mod = _module(dev)
        data = {k: (v if k in ("intrinsics", "extrinsics") else v.to(dev)) for k, v in host.items()}
        steps[n] = TrainStep(mod, data, lr=mod.cfg.learning_rate, weight_decay=mod.cfg.weight_decay,
                             graph=True, warmup=2, **OPT[n])
    fns = {n: _block(s, a.step_block) for n, s in steps.items()}
    fns["off2"] = fns["off"]
    res = _alternate(fns, a.step_blocks)
    for n in res:
        if n != "off":
            res[n]["minus_off_ms"] = round(res[n]["median_ms"] - res["off"]["median_ms"], 4)
    res["off_spread_ms"] = round(res["off"]["max_ms"] - res["off"]["min_ms"], 4)
    res["config"] = (f"TrainStep (fwd + 3 losses + bwd + Adam), B={a.batch}, 4x256^2, fp32, captured; "
                     f"ms per call, {a.step_block} calls per block")
    if "ema" in steps:
        res["ema_updates"] = int(steps["ema"].opt.ema_updates_dev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="optimizer calls per block")
    ap.add_argument("--blocks", type=int, default=9, help="timed blocks per optimizer setting")
    ap.add_argument("--step-block", type=int, default=10, help="train-step calls per block")
    ap.add_argument("--step-blocks", type=int, default=12, help="timed blocks per train step")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--baseline", action="store_true",
                    help="the settings without the average only (runs on the parent commit too)")
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from e2ep_amd import _lib
    _lib.load()
    dev = torch.device("cuda")
    res = {"baseline_only": a.baseline, "device": torch.cuda.get_device_name(0)}
    res["optimizer"] = bench_optimizer(a, dev, ["off", "clip"] if a.baseline
                                       else ["off", "ema", "clip", "ema_clip"])
    if not a.no_train_step:
        res["train_step"] = bench_train_step(a, dev, ["off"] if a.baseline else ["off", "ema"])
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
