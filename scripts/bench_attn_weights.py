"""Cost of the closed-loop agent's attention-map capture on ParkingModel.predict at B=1.

The agent patches the last encoder layer's self_attn to return per-head attention weights and
hooks its output (agent/parking_agent.py:71-91,266-268).  This times, in ONE process and
alternating the variants call by call (so clock and thermal drift hit all of them alike), the
captured predict

    (a) un-hooked                                   (measured twice per round: a, a2 — the
                                                     difference of their medians is the spread
                                                     the other differences are read against)
    (b) hooked, weights from e2ep_attn_weights      (attention.MultiheadAttention's fused forward)
    (c) hooked, the fused forward switched off      (E2EP_ATTN_WEIGHTS=0: torch's own
                                                     MultiheadAttention.forward, bmm / softmax / bmm)

each call synchronised, the per-call inputs copied into the static buffers on the stream and
included in the timing (as scripts/bench_predict.py).

    python scripts/bench_attn_weights.py [--iters 200] [--precision fp16] [--json out.json]
    python scripts/bench_attn_weights.py --only b --iters 20     # one variant (for a profiler)
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


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts) * 1e3, q)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--precision", choices=("fp32", "fp16", "bf16"), default="fp32")
    ap.add_argument("--only", choices=("a", "b", "c"), default=None)
    a = ap.parse_args()
    from e2ep_amd import _lib, attention, graphs, precision, synthetic
    from model.parking_model import ParkingModel
    from tool.config import default_cfg

    _lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m = ParkingModel(default_cfg()).to(dev).eval()
    host = synthetic.synthetic_batch(1, seed=0)
    host["gt_control"] = host["gt_control"][:, :1]  # BOS: the agent's first token
    keys = ("image", "target_point", "ego_motion", "gt_control")
    static = {k: host[k].to(dev) for k in keys}
    static["intrinsics"], static["extrinsics"] = host["intrinsics"], host["extrinsics"]
    noise = synthetic.target_noise(1, seed=0).to(dev)
    precision.set(a.precision)

    def call():
        with torch.no_grad():
            return m.predict(static, noise)

    def capture():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                call()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        return graphs.capture(call)

    want = ("a", "b", "c") if a.only is None else (a.only,)
    graph, outs, seen = {}, {}, {}
    if "a" in want:
        graph["a"], outs["a"], _ = capture()
    # the agent's patch and hook, restated
    sa = m.feature_fusion.tf_encoder.layers[-1].self_attn
    forward_orig = sa.forward

    def wrap(*args, **kwargs):
        kwargs["need_weights"] = True
        kwargs["average_attn_weights"] = False
        return forward_orig(*args, **kwargs)
    sa.forward = wrap
    saved = []
    sa.register_forward_hook(lambda mod, args, out: saved.append(out[1]))
    for name, fused in (("b", True), ("c", False)):
        if name not in want:
            continue
        attention._FUSED_FORWARD[0] = fused
        graph[name], outs[name], _ = capture()
        seen[name] = saved[-1]
    attention._FUSED_FORWARD[0] = True

    order = [n for n in ("a", "b", "c") if n in graph] + (["a2"] if "a" in graph else [])
    times = {n: [] for n in order}
    for it in range(a.iters + 10):
        for n in order:
            t0 = time.perf_counter()
            for k in keys:
                static[k].copy_(host[k], non_blocking=True)
            graph["a" if n == "a2" else n].replay()
            torch.cuda.synchronize()
            if it >= 10:  # the first rounds warm up
                times[n].append(time.perf_counter() - t0)
    precision.set("fp32")

    res = {"config": f"ParkingModel.predict, B=1, captured, conv GEMM operands {a.precision}; "
                     "a = un-hooked (a2 = its repeat), b = hooked on e2ep_attn_weights, "
                     "c = hooked on torch's MultiheadAttention.forward",
           "precision": a.precision, "iters": a.iters}
    for n in order:
        res[f"{n}_p50_ms"], res[f"{n}_p90_ms"] = pct(times[n], 50), pct(times[n], 90)
    if "a2" in times:
        res["spread_ms"] = round(abs(res["a_p50_ms"] - res["a2_p50_ms"]), 4)
    if "a" in graph and "b" in graph:
        res["b_minus_a_ms"] = round(res["b_p50_ms"] - res["a_p50_ms"], 4)
        res["tokens_b_equal_a"] = bool(torch.equal(outs["b"][0], outs["a"][0]))
    if "b" in graph and "c" in graph:
        res["b_minus_c_ms"] = round(res["b_p50_ms"] - res["c_p50_ms"], 4)
        d = (seen["b"].double() - seen["c"].double()).norm() / seen["c"].double().norm()
        res["weights_b_vs_c_rel_l2"] = float(d)
        res["weights_shape"] = list(seen["b"].shape)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
