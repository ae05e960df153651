"""Time of one validation batch (ParkingModel, B = 8, 4 x 256^2, fp32): the module's eager
validation_step against ValStep, eager and captured.

ONE process, one module (eval mode, fixed weights), one batch and noise on the device; the
settings are called in alternating blocks so clock and thermal drift hit them alike:

    eager          module.validation_step under no_grad (the eval forward launch by launch,
                   ControlValLoss as a chain of torch ops, Python's sum), nothing read back
    eager2         the same again: a second series of the baseline, so the difference between
                   two series of ONE setting is on the table next to the differences between
                   settings
    valstep_eager  ValStep(graph=False): the e2ep metric kernels and the device accumulator,
                   the forward still launch by launch
    valstep_graph  ValStep(graph=True): one replayed HIP graph
    valstep_eager_depth, valstep_graph_depth  (--depth-metrics only) the same two with
                   depth_metrics=True: two more launches after the depth loss; the feature's cost
                   per batch is valstep_graph_depth - valstep_graph of the same series

    --rollout      instead of the above, three captured settings only: valstep_graph,
                   valstep_graph_rollout (ValStep(rollout=True): the forward also decodes every
                   control token from BOS through the KV-cached ar_decode, and two launches
                   score the tokens) and valstep_graph_rollout_fullpass (the same with the decode
                   cache off when the step is captured, ar_decode._DECODE_CACHE: the full
                   decoder pass per token); the rollout's cost per batch is
                   valstep_graph_rollout - valstep_graph of the same series

A block is `--block` calls, synchronised once at its end; its figure is ms per call.  Per
setting: the median over blocks and their spread (min, max).  Launches are not traced.  The
e2ep launches of the metric chain are counted on one eager ValStep call (entry-point calls
times the kernels behind each, LAUNCHES below); the torch kernels ControlValLoss and sum()
launch are an ASSUMED count read off loss/control_loss.py; the result line says so
(launch_count_basis).

    python scripts/bench_val.py [--blocks 12] [--block 10] [--depth-metrics | --rollout]
                                [--json out.json]
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

# kernel launches behind one call of a metric entry point (csrc/val.hip, csrc/loss.hip)
LAUNCHES = {"e2ep_control_val_fwd": 2, "e2ep_seg_confusion": 2, "e2ep_val_accumulate": 1,
            "e2ep_seg_ce_fwd": 2, "e2ep_depth_bce_fwd": 2, "e2ep_depth_bce_fwd_f64": 2,
            "e2ep_depth_metrics": 2, "e2ep_depth_metrics_f64": 2, "e2ep_rollout_metrics": 2}
# ControlValLoss.forward as torch kernels, assumed one per op: 3 softmax, 2 argmax, 1 float
# cast, acc: gt, 2 x (div, sub), neg, where; steer: div, sub; 2 x smooth_l1 (+ 2 reshape
# copies of the strided argmax results); 2 partial sums, stack, CE on the transposed pair
# (a contiguous copy, log_softmax, nll_loss); acc + steer; then sum(d.values()): 0 + a and
# three more adds
ASSUMED_TORCH_KERNELS = 3 + 2 + 1 + 1 + 4 + 1 + 1 + 2 + 2 + 2 + 2 + 1 + 3 + 1 + 4


def _setup(a):
    from e2ep_amd import _lib, synthetic
    from tool.config import default_cfg
    from trainer.pl_trainer import ParkingTrainingModule

    _lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(1234)
    mod = ParkingTrainingModule(default_cfg()).to(dev).eval()
    host = synthetic.synthetic_batch(a.batch, seed=0)
    data = {k: (v if k in ("intrinsics", "extrinsics") else v.to(dev)) for k, v in host.items()}
    return mod, data, synthetic.target_noise(a.batch, seed=0).to(dev)


def _stats(t):
    t = np.asarray(t)
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
            "max_ms": round(float(t.max()), 4), "blocks_ms": [round(float(x), 4) for x in t]}


def rollout(a):
    """--rollout: the three captured settings in alternating blocks."""
    from e2ep_amd import ar_decode
    from e2ep_amd.val import ValStep
    mod, data, noise = _setup(a)
    steps = {"valstep_graph": ValStep(mod, data, noise=noise, graph=True, warmup=2)}
    before = ar_decode.LAUNCHES[0]
    steps["valstep_graph_rollout"] = ValStep(mod, data, noise=noise, graph=True, warmup=2,
                                             rollout=True)
    kv_launches = (ar_decode.LAUNCHES[0] - before) // 3  # two warm-up runs and the capture
    ar_decode._DECODE_CACHE[0] = False  # the path is fixed when the step is captured
    try:
        steps["valstep_graph_rollout_fullpass"] = ValStep(mod, data, noise=noise, graph=True,
                                                          warmup=2, rollout=True)
    finally:
        ar_decode._DECODE_CACHE[0] = True

    def block(name):
        v = steps[name]
        t0 = time.perf_counter()
        for _ in range(a.block):
            v()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.block * 1e3

    order = list(steps)
    for n in order:
        block(n)
    for v in steps.values():
        v.reset()
    times = {n: [] for n in order}
    for r in range(a.blocks):
        for n in order[r % len(order):] + order[:r % len(order)]:  # rotate who goes first
            times[n].append(block(n))
    res = {"config": f"one validation batch (eval fwd + 4 losses + metrics), B={a.batch}, "
                     "4x256^2, fp32, captured; ms per call, one figure per block",
           "blocks_per_setting": a.blocks, "calls_per_block": a.block}
    for n in order:
        res[n] = _stats(times[n])
        res[f"{n}_spread_ms"] = round(res[n]["max_ms"] - res[n]["min_ms"], 4)
    base = res["valstep_graph"]["median_ms"]
    res["rollout_cost_graph_ms"] = round(res["valstep_graph_rollout"]["median_ms"] - base, 4)
    res["rollout_fullpass_cost_graph_ms"] = round(
        res["valstep_graph_rollout_fullpass"]["median_ms"] - base, 4)
    res["dec_launches_per_call"] = kv_launches
    out = {n: v.result() for n, v in steps.items()}
    res["batches_accumulated"] = [out[n]["batches"] for n in order]
    res["val_loss_mean"] = [out[n]["val_loss"] for n in order]
    kv, full = steps["valstep_graph_rollout"], steps["valstep_graph_rollout_fullpass"]
    res["rollout_tokens_equal_fullpass"] = bool(torch.equal(kv.rollout_tokens, full.rollout_tokens))
    res["rollout_metrics"] = {k: np.asarray(v).tolist() for k, v in out["valstep_graph_rollout"].items()
                              if k.startswith("rollout_")}
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=12, help="timed blocks per setting")
    ap.add_argument("--block", type=int, default=10, help="calls per block")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--depth-metrics", action="store_true",
                    help="add the two ValStep settings with depth_metrics=True")
    ap.add_argument("--rollout", action="store_true",
                    help="time valstep_graph against the two captured rollout=True settings only")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.rollout:
        return rollout(a)
    from e2ep_amd import _lib, synthetic
    from e2ep_amd.val import ValStep
    from tool.config import default_cfg
    from trainer.pl_trainer import ParkingTrainingModule

    _lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(1234)
    mod = ParkingTrainingModule(default_cfg()).to(dev).eval()
    host = synthetic.synthetic_batch(a.batch, seed=0)
    data = {k: (v if k in ("intrinsics", "extrinsics") else v.to(dev)) for k, v in host.items()}
    noise = synthetic.target_noise(a.batch, seed=0).to(dev)
    v_eager = ValStep(mod, data, noise=noise, graph=False)
    v_graph = ValStep(mod, data, noise=noise, graph=True, warmup=2)

    def eager():
        with torch.no_grad():
            mod.validation_step(data, 0, noise)

    calls = {"eager": eager, "eager2": eager, "valstep_eager": lambda: v_eager(),
             "valstep_graph": lambda: v_graph()}
    if a.depth_metrics:
        v_eager_d = ValStep(mod, data, noise=noise, graph=False, depth_metrics=True)
        v_graph_d = ValStep(mod, data, noise=noise, graph=True, warmup=2, depth_metrics=True)
        calls["valstep_eager_depth"] = lambda: v_eager_d()
        calls["valstep_graph_depth"] = lambda: v_graph_d()

    def block(name):
        fn = calls[name]
        t0 = time.perf_counter()
        for _ in range(a.block):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.block * 1e3

    order = list(calls)
    for n in order:  # warm-up: code objects, caches and buffers, clocks settled
        block(n)
    v_eager.reset()
    v_graph.reset()
    if a.depth_metrics:
        v_eager_d.reset()
        v_graph_d.reset()
    times = {n: [] for n in order}
    for r in range(a.blocks):
        for n in order[r % len(order):] + order[:r % len(order)]:  # rotate who goes first
            times[n].append(block(n))

    # the metric chain's e2ep launches, counted on one more eager ValStep call
    count, orig = [0], _lib.call

    def counted(name, *args):
        count[0] += LAUNCHES.get(name, 0)
        return orig(name, *args)
    _lib.call = counted
    try:
        v_eager()
    finally:
        _lib.call = orig
    torch.cuda.synchronize()

    res = {"config": f"one validation batch (eval fwd + 4 losses + metrics), B={a.batch}, "
                     "4x256^2, fp32; ms per call, one figure per block",
           "blocks_per_setting": a.blocks, "calls_per_block": a.block}
    for n in order:
        t = np.asarray(times[n])
        res[n] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
                  "max_ms": round(float(t.max()), 4), "blocks_ms": [round(float(x), 4) for x in t]}
    for n in order[1:]:
        res[f"{n}_minus_eager_ms"] = round(res[n]["median_ms"] - res["eager"]["median_ms"], 4)
    res["eager_spread_ms"] = round(res["eager"]["max_ms"] - res["eager"]["min_ms"], 4)
    res["valstep_metric_launches_per_call"] = count[0]
    res["eager_metric_launches_per_call_assumed"] = ASSUMED_TORCH_KERNELS + 4
    res["launch_count_basis"] = (
        "not traced: ValStep's figure is the e2ep entry-point calls of one eager call after the "
        "timed blocks (forward excluded) times the kernels each launches (LAUNCHES, from "
        "csrc/val.hip and csrc/loss.hip); the eager figure is the 4 launches of the two e2ep "
        "losses plus an ASSUMED one torch kernel per op of ControlValLoss.forward and of "
        "sum(d.values()) (ASSUMED_TORCH_KERNELS, read off loss/control_loss.py)")
    r_e, r_g = v_eager.result(), v_graph.result()
    res["batches_accumulated"] = [r_e["batches"], r_g["batches"]]
    res["val_loss_mean"] = [r_e["val_loss"], r_g["val_loss"]]
    res["eager_val_loss"] = float(mod.logged["val_loss"])
    res["seg_miou"] = r_g["seg_miou"]
    if a.depth_metrics:
        count[0] = 0
        _lib.call = counted
        try:
            v_eager_d()
        finally:
            _lib.call = orig
        torch.cuda.synchronize()
        res["valstep_depth_metric_launches_per_call"] = count[0]
        res["depth_cost_graph_ms"] = round(res["valstep_graph_depth"]["median_ms"]
                                           - res["valstep_graph"]["median_ms"], 4)
        res["depth_cost_eager_ms"] = round(res["valstep_eager_depth"]["median_ms"]
                                           - res["valstep_eager"]["median_ms"], 4)
        res["valstep_graph_spread_ms"] = round(res["valstep_graph"]["max_ms"]
                                               - res["valstep_graph"]["min_ms"], 4)
        res["valstep_graph_depth_spread_ms"] = round(res["valstep_graph_depth"]["max_ms"]
                                                     - res["valstep_graph_depth"]["min_ms"], 4)
        r_d = v_graph_d.result()
        res["val_loss_mean_depth"] = [v_eager_d.result()["val_loss"], r_d["val_loss"]]
        res["depth_metrics"] = {k: v for k, v in r_d.items()
                                if k.startswith("depth_") and k != "depth_per_camera"}
        res["depth_bin_acc_per_camera"] = r_d["depth_per_camera"]["depth_bin_acc"].tolist()
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
