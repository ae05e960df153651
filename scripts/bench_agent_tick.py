"""The agent's whole tick at B = 1 (config C5: conv GEMM operands fp16): the host chain the
reference agent runs around the captured ParkingModel.predict against AgentStep
(e2ep_amd/agent_step.py), which moves that chain onto the device.

ONE process; the settings run in alternating blocks (clock and thermal drift hit them alike),
every tick ending in a synchronisation:

    host_vec    ProcessImage x 4, torch.cat, fp32 H2D -> captured predict -> torch.argmax ->
                .cpu() -> the vectorised NumPy centroid (as tests/agent_ref.py) -> detokenize;
                the fed-back target point goes through the host.  The fair baseline.
    host_scan   the same with the per-pixel interpreted scan of all 40 000 pixels instead of
                the vectorised centroid: what the reference agent ships
                (agent/parking_agent.py:298-305), restated
    host_vec2   host_vec again: |p50(host_vec) - p50(host_vec2)| is the noise floor
    agent_step  AgentStep.tick: one H2D of raw bytes, one graph replay, one small D2H, one sync

    python scripts/bench_agent_tick.py [--iters 200] [--block 20] [--json out.json]
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "e2e-parking-carla_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, N_CAMS, N_FRAMES = 300, 400, 4, 8


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts) * 1e3, q)), 4)


def scan_centroid(seg_img, res):
    """The interpreted per-pixel scan, on the flipped 0 / 128 / 255 image."""
    h, w = seg_img.shape
    xs, ys = [], []
    for r in range(h):
        for c in range(w):
            if seg_img[r, c] == 255:
                xs.append(r)
                ys.append(c)
    if not xs:
        return None
    tx, ty = int(np.average(xs)), int(np.average(ys))
    return [-(tx - h / 2) * res[0], (ty - h / 2) * res[1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="timed ticks per setting")
    ap.add_argument("--block", type=int, default=20, help="ticks per block of one setting")
    ap.add_argument("--json", default=None)
    ap.add_argument("--precision", choices=("fp32", "fp16"), default="fp16")
    a = ap.parse_args()
    from dataset.carla_dataset import ProcessImage, detokenize
    from e2ep_amd import _lib, agent_step, graphs, precision, synthetic
    from model.parking_model import ParkingModel
    from tool.config import default_cfg

    _lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    cfg = default_cfg()
    m = ParkingModel(cfg).to(dev).eval()
    K, E = synthetic.rig(N_CAMS, cfg.image_crop)
    K, E = K[None], E[None]
    noise = synthetic.target_noise(1, seed=0)
    res = (cfg.bev_x_bound[2], cfg.bev_y_bound[2])
    ticks = []
    for k in range(N_FRAMES):
        raw = np.random.RandomState(k).randint(0, 256, (N_CAMS, H, W, 4)).astype(np.uint8)
        b = synthetic.synthetic_batch(1, seed=100 + k)
        ticks.append(dict(
            frames=[types.SimpleNamespace(raw_data=f.tobytes(), height=H, width=W) for f in raw],
            ego=b["ego_motion"][0, 0].tolist(), goal=b["target_point"][0].tolist()))
    precision.set(a.precision)

    # let class 2 win on about a seventh of the map, so every setting walks the found branch
    image0, _ = agent_step.decode_bgra(torch.from_numpy(np.stack(
        [np.frombuffer(f.raw_data, np.uint8).reshape(H, W, 4) for f in ticks[0]["frames"]])).to(dev),
        cfg.image_crop)
    static = {"image": image0.view(1, N_CAMS, 3, cfg.image_crop, cfg.image_crop).clone(),
              "target_point": torch.tensor([ticks[0]["goal"]], device=dev),
              "ego_motion": torch.tensor([[ticks[0]["ego"]]], device=dev),
              "gt_control": torch.tensor([[cfg.token_nums - 3]], device=dev),
              "intrinsics": K, "extrinsics": E}
    snoise = noise.to(dev)
    with torch.no_grad():
        seg = m.predict(static, snoise)[1][0]
        gap = torch.maximum(seg[0], seg[1]) - seg[2]
        m.segmentation_head.segmentation_head[3].bias[2] += torch.quantile(gap.flatten(), 0.15)

    def call():
        with torch.no_grad():
            return m.predict(static, snoise)

    def count_calls(fn):
        n, orig = [0], _lib.call

        def counted(*args):
            n[0] += 1
            return orig(*args)
        _lib.call = counted
        try:
            fn()
            return n[0]
        finally:
            _lib.call = orig

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g, gout, _ = graphs.capture(call)
    predict_calls = count_calls(call)

    proc = ProcessImage(cfg.image_crop)
    prev = {"host_vec": None, "host_scan": None}

    def host_tick(t, scan):
        key = "host_scan" if scan else "host_vec"
        # get_model_data (agent/parking_agent.py:456-478)
        images = torch.cat([proc(f)[0] for f in t["frames"]], dim=0).unsqueeze(0)
        target = list(t["goal"])
        if prev[key] is not None:
            target = [prev[key][0], prev[key][1], target[2]]
        static["image"].copy_(images, non_blocking=True)
        static["target_point"].copy_(torch.tensor(target, dtype=torch.float).unsqueeze(0), non_blocking=True)
        static["ego_motion"].copy_(torch.tensor(t["ego"], dtype=torch.float).view(1, 1, 3), non_blocking=True)
        g.replay()
        toks, seg = gout[0], gout[1]
        # save_prev_target (:290-311) and detokenize (:391)
        cls = torch.argmax(seg[0], dim=0, keepdim=True).detach().cpu().numpy()
        if scan:
            cls[cls == 1] = 128
            cls[cls == 2] = 255
            p = scan_centroid(cls[0][::-1], res)
        else:
            flipped = cls[0][::-1]
            rows, cols = np.nonzero(flipped == 2)
            p = None
            if rows.size:
                tx, ty = int(rows.sum()) // rows.size, int(cols.sum()) // rows.size
                hh = flipped.shape[0]
                p = [-(tx - hh / 2) * res[0], (ty - hh / 2) * res[1]]
        if p is not None:
            prev[key] = p
        tokens = toks[0].tolist()
        return detokenize(tokens[1:], cfg.token_nums), tokens, prev[key]

    step = agent_step.AgentStep(m, cam_hw=(H, W), n_cams=N_CAMS)

    def agent_tick(t):
        r = step.tick(t["frames"], t["ego"], t["goal"], K, E, noise=noise)
        return r.controls, r.tokens, r.next_target

    # the same trajectory from a cleared start: equal tokens, controls and fed-back points
    same = True
    for t in ticks:
        hv, hs, ag = host_tick(t, False), host_tick(t, True), agent_tick(t)
        pt = lambda p: None if p is None else [float(np.float32(v)) for v in p]  # noqa: E731
        same = same and hv[:2] == hs[:2] == ag[:2] and pt(hv[2]) == pt(hs[2]) == pt(ag[2])
    found = prev["host_vec"] is not None
    eager = agent_step.AgentStep(m, cam_hw=(H, W), n_cams=N_CAMS, capture=False)
    eager.tick(ticks[0]["frames"], ticks[0]["ego"], ticks[0]["goal"], K, E, noise=noise)
    step_calls = count_calls(eager._run)

    runners = {"host_vec": lambda t: host_tick(t, False), "host_scan": lambda t: host_tick(t, True),
               "host_vec2": lambda t: host_tick(t, False), "agent_step": agent_tick}
    order = list(runners)
    times = {n: [] for n in order}
    i = [0]

    def one(n):
        t = ticks[i[0] % N_FRAMES]
        i[0] += 1
        t0 = time.perf_counter()
        runners[n](t)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for n in order:
        for _ in range(10):
            one(n)
    rounds = -(-a.iters // a.block)
    for r in range(rounds):
        for n in order[r % len(order):] + order[:r % len(order)]:
            for j in range(a.block + 2):
                t = one(n)
                if j >= 2:
                    times[n].append(t)
    precision.set("fp32")

    out = {"config": f"agent tick, B=1, {N_CAMS} cams {H}x{W} BGRA -> crop {cfg.image_crop}, captured "
                     f"predict, conv GEMM operands {a.precision}",
           "ticks_per_setting": rounds * a.block, "block": a.block,
           "trajectories_equal": bool(same), "slot_found_in_trajectory": bool(found),
           "e2ep_calls_predict": predict_calls, "e2ep_calls_agent_step": step_calls,
           "e2ep_calls_added_by_the_tick": step_calls - predict_calls}
    for n in order:
        out[f"{n}_p50_ms"], out[f"{n}_p90_ms"] = pct(times[n], 50), pct(times[n], 90)
    out["noise_floor_ms"] = round(abs(out["host_vec_p50_ms"] - out["host_vec2_p50_ms"]), 4)
    out["agent_step_minus_host_vec_ms"] = round(out["agent_step_p50_ms"] - out["host_vec_p50_ms"], 4)
    out["agent_step_minus_host_scan_ms"] = round(out["agent_step_p50_ms"] - out["host_scan_p50_ms"], 4)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
