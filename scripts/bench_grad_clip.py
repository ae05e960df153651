"""Cost of gradient-norm clipping, non-finite-step skipping and gradient accumulation on the
captured C2 train step (ParkingModel, B = 8, 4 x 256^2, fp32; bench.py's workload).

ONE process; one captured TrainStep per setting (each with its own module, same initial
weights and batch), called in alternating blocks so clock and thermal drift hit them alike:

    off    no option: the parent's graphs and launches
    clip   max_grad_norm=1.0, skip_nonfinite=True
    acc2   the same with accumulate=2 (every call is one micro-step; every second one updates)
    off2   the off step again: a second series of the baseline, so the difference between two
           series of ONE setting is on the table next to the differences between settings

A block is `--block` calls, synchronised once at its end; its figure is ms per call.  Per
setting: the median over blocks and their spread (min, max).  Launches added per call are not
traced: they are the e2ep entry-point calls one eager update makes times the kernels behind
each (LAUNCHES below), plus an assumed count for the torch kernels of FlatAdam.has_grad (ne +
copy, and a maximum for the union); the result line says so (launch_count_basis).

    python scripts/bench_grad_clip.py [--blocks 12] [--block 10] [--json out.json]
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

# kernel launches behind one call of an optimizer entry point (csrc/adam.hip)
LAUNCHES = {"e2ep_adam_step": 2, "e2ep_adam_step_clipped": 2, "e2ep_grad_sqnorm": 1,
            "e2ep_grad_norm_finalize": 1, "e2ep_grad_gather": 1, "e2ep_grad_accumulate": 1}
SETTINGS = {"off": {}, "clip": dict(max_grad_norm=1.0, skip_nonfinite=True),
            "acc2": dict(max_grad_norm=1.0, skip_nonfinite=True, accumulate=2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=12, help="timed blocks per setting")
    ap.add_argument("--block", type=int, default=10, help="calls per block (even)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from e2ep_amd import _lib, synthetic
    from e2ep_amd.train import TrainStep
    from tool.config import default_cfg
    from trainer.pl_trainer import ParkingTrainingModule

    _lib.load()
    dev = torch.device("cuda")
    host = synthetic.synthetic_batch(a.batch, seed=0)
    steps = {}
    for name, kw in SETTINGS.items():
        torch.manual_seed(1234)
        mod = ParkingTrainingModule(default_cfg()).to(dev).train()
        for p in mod.parking_model.bev_encoder.layer4.parameters():
            p.requires_grad_(False)
        data = {k: (v if k in ("intrinsics", "extrinsics") else v.to(dev)) for k, v in host.items()}
        steps[name] = TrainStep(mod, data, lr=mod.cfg.learning_rate,
                                weight_decay=mod.cfg.weight_decay, graph=True, warmup=2, **kw)

    def optimizer_launches(step):
        """Launches of the optimizer side of one call, averaged over an accumulation cycle,
        counted on the eager functions the graphs were captured from.  (It runs one more
        update on the gradients of the last call.)"""
        n, orig = [0], _lib.call

        def counted(name, *args):
            n[0] += LAUNCHES.get(name, 0)
            return orig(name, *args)
        _lib.call = counted
        try:
            if step.accumulate > 1:
                step._accumulate(True)
                for _ in range(step.accumulate - 1):
                    step._accumulate(False)
                n[0] += 2 + 3 * (step.accumulate - 1)  # has_grad's torch kernels
            step._update()
        finally:
            _lib.call = orig
        torch.cuda.synchronize()
        return n[0] / step.accumulate

    def block(name):
        s = steps["off" if name == "off2" else name]
        t0 = time.perf_counter()
        for _ in range(a.block):
            s()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.block * 1e3

    order = ["off", "clip", "acc2", "off2"]
    for n in order:  # warm-up: every graph's code objects and buffers, clocks settled
        block(n)
    times = {n: [] for n in order}
    for r in range(a.blocks):
        for n in order[r % len(order):] + order[:r % len(order)]:  # rotate who goes first
            times[n].append(block(n))
    launches = {n: optimizer_launches(s) for n, s in steps.items()}

    res = {"config": f"TrainStep (fwd + 3 losses + bwd + Adam), B={a.batch}, 4x256^2, fp32, "
                     "captured; ms per call, one figure per block",
           "blocks_per_setting": a.blocks, "calls_per_block": a.block}
    for n in order:
        t = np.asarray(times[n])
        res[n] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
                  "max_ms": round(float(t.max()), 4), "blocks_ms": [round(float(x), 4) for x in t]}
    for n in ("clip", "acc2", "off2"):
        res[f"{n}_minus_off_ms"] = round(res[n]["median_ms"] - res["off"]["median_ms"], 4)
    res["off_spread_ms"] = round(res["off"]["max_ms"] - res["off"]["min_ms"], 4)
    res["launch_count_basis"] = (
        "not traced: e2ep entry-point calls of one eager gather / accumulate / update after the "
        "timed blocks (one extra update per setting), times the kernels each entry point "
        "launches (LAUNCHES, from csrc/adam.hip), plus an ASSUMED 2 torch kernels per "
        "FlatAdam.has_grad call (ne, copy) and 3 with union=True (ne, copy, maximum)")
    for n, v in launches.items():
        res[f"{n}_optimizer_launches_per_call"] = v
        res[f"{n}_launches_added_per_call"] = v - launches["off"]
    for n in ("clip", "acc2"):
        o = steps[n].opt
        res[f"{n}_grad_norm"], res[f"{n}_clip_coef"] = float(o.grad_norm_dev), float(o.clip_coef_dev)
        res[f"{n}_skipped"] = int(o.skipped_dev)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
