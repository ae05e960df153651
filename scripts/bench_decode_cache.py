"""A/B of the KV-cached incremental control-token decode (E2EP_DECODE_CACHE, e2ep_amd/
ar_decode.py) on the captured ParkingModel.predict at B = 1, as the closed-loop agent runs it
(config C5: conv GEMM operands fp16).

ONE process; the predict is captured once per switch setting and the settings are replayed in
alternating blocks (so clock and thermal drift hit them alike):

    off   the full decoder pass per generated token (the parent's path)
    on    the incremental path
    off2  the off graph again: |p50(off) - p50(off2)| is the noise floor the difference
          on - off is read against

each replay synchronised, the per-call inputs copied into the static buffers on the stream and
included in the timing (as scripts/bench_attn_weights.py).

    python scripts/bench_decode_cache.py [--iters 250] [--block 25] [--json out.json]
    python scripts/bench_decode_cache.py --only on --iters 20     # one setting (for a profiler)
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
    ap.add_argument("--iters", type=int, default=250, help="timed replays per setting (>= 200)")
    ap.add_argument("--block", type=int, default=25, help="replays per block of one setting")
    ap.add_argument("--json", default=None)
    ap.add_argument("--precision", choices=("fp32", "fp16"), default="fp16")
    ap.add_argument("--only", choices=("on", "off"), default=None)
    a = ap.parse_args()
    from e2ep_amd import _lib, ar_decode, graphs, precision, synthetic
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

    def count_calls():
        """e2ep entry-point calls (launches, nearly one to one) of one eager predict."""
        n, orig = [0], _lib.call

        def counted(*args):
            n[0] += 1
            return orig(*args)
        _lib.call = counted
        try:
            d0 = ar_decode.LAUNCHES[0]
            call()
            return n[0], ar_decode.LAUNCHES[0] - d0
        finally:
            _lib.call = orig

    def capture():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                call()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        return graphs.capture(call)

    want = ("off", "on") if a.only is None else (a.only,)
    graph, outs, calls = {}, {}, {}
    for name in want:
        ar_decode._DECODE_CACHE[0] = name == "on"
        graph[name], outs[name], _ = capture()
        calls[name] = count_calls()
    ar_decode._DECODE_CACHE[0] = True

    def replay(n):
        t0 = time.perf_counter()
        for k in keys:
            static[k].copy_(host[k], non_blocking=True)
        graph["off" if n == "off2" else n].replay()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    order = [n for n in ("off", "on") if n in graph] + (["off2"] if "off" in graph else [])
    times = {n: [] for n in order}
    for n in order:  # warm-up: every graph's code objects and buffers, clocks settled
        for _ in range(30):
            replay(n)
    rounds = -(-a.iters // a.block)
    for r in range(rounds):
        for n in order[r % len(order):] + order[:r % len(order)]:  # rotate who goes first
            for i in range(a.block + 2):
                t = replay(n)
                if i >= 2:  # the first replays after a switch of graphs are not kept
                    times[n].append(t)
    precision.set("fp32")

    res = {"config": f"ParkingModel.predict, B=1, captured, conv GEMM operands {a.precision}; "
                     "off = full decoder pass per token (off2 = its repeat), on = KV-cached "
                     "incremental decode",
           "precision": a.precision, "replays_per_setting": rounds * a.block, "block": a.block}
    for n in order:
        res[f"{n}_p50_ms"], res[f"{n}_p90_ms"] = pct(times[n], 50), pct(times[n], 90)
    for n in graph:
        res[f"{n}_e2ep_calls_per_predict"], res[f"{n}_dec_launches_per_predict"] = calls[n]
    if "off2" in times:
        res["noise_floor_ms"] = round(abs(res["off_p50_ms"] - res["off2_p50_ms"]), 4)
    if "on" in graph and "off" in graph:
        res["on_minus_off_ms"] = round(res["on_p50_ms"] - res["off_p50_ms"], 4)
        res["tokens_on_equal_off"] = bool(torch.equal(outs["on"][0], outs["off"][0]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
