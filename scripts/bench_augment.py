"""Cost of the photometric augmentation of the GPU frame decode (e2ep_amd/augment.py,
csrc/decode.hip k_decode_frames_aug + e2ep_frame_gray_mean).

ONE process, two parts, every setting timed in alternating blocks so clock and thermal drift
hit them alike; per setting the median over blocks and their spread (min, max).  The bar is
`off`, the un-augmented path of the same build (the parent's code), and `off2` is `off` a
second time: two series of ONE setting next to every difference.

A. The loader: GpuFrameLoader samples/s at --batch over a synthetic cache (random uint8 frames
   in the cache's own layout, --samples of them), streamed and resident, augment None (off,
   off2) and a PhotoAugment with every effect on (on).  A block is --epochs epochs,
   synchronised at its end.

B. The launches alone, HIP events around --iters back-to-back calls of the C entry points on
   staged device tables (no Python argument handling inside the window), one batch of --batch
   samples gathered out of the resident cache:
       off / off2   e2ep_decode_frames                               26 B per camera pixel
       aug          e2ep_decode_frames_aug alone (pivot precomputed)  26 B
       mean         e2ep_frame_gray_mean alone (memset + 2 launches)   3 B
       on           mean + aug, what an augmented batch launches      29 B
   `gbps` is the byte model over the median time.

    python scripts/bench_augment.py [--samples 256] [--rounds 7] [--json out.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "e2e-parking-carla_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

BYTES = {"off": 26, "off2": 26, "aug": 26, "mean": 3, "on": 29}


def _stats(v, unit):
    v = np.asarray(v)
    return {f"median_{unit}": round(float(np.median(v)), 4), f"min_{unit}": round(float(v.min()), 4),
            f"max_{unit}": round(float(v.max()), 4), "blocks": [round(float(x), 4) for x in v]}


def _alternate(fns, rounds):
    """fns: name -> callable returning one block's figure.  One warm-up block each, then
    `rounds` rounds, rotating who goes first."""
    order = list(fns)
    for n in order:
        fns[n]()
    out = {n: [] for n in order}
    for r in range(rounds):
        k = r % len(order)
        for n in order[k:] + order[:k]:
            out[n].append(fns[n]())
    return out


def synthetic_cache(path, samples, crop):
    """A FrameCache of random frames and labels, written in the cache's own layout."""
    from dataset import frame_cache as fc
    g = np.random.default_rng(0)
    layout = fc._layout(samples, crop, 15, 4)
    os.makedirs(path, exist_ok=True)
    for name, (dt, shape) in layout.items():
        if np.dtype(dt) == np.uint8:
            a = g.integers(0, 3 if name == "bev" else 256, shape, dtype=np.uint8)
        else:
            a = g.integers(0, 2, shape).astype(dt)
        np.save(os.path.join(path, name + ".npy"), a)
    meta = {"version": fc.VERSION, "samples": samples, "image_crop": crop, "bev": fc.BEV,
            "intrinsics": np.tile(np.eye(3), (4, 1, 1)).tolist(),
            "extrinsics": np.tile(np.eye(4), (4, 1, 1)).tolist(), "fingerprint": "synthetic",
            "fields": {f: [np.dtype(dt).str, list(shape)] for f, (dt, shape) in layout.items()}}
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump(meta, f)
    return fc.FrameCache(path)


def bench_loader(a, cache, aug):
    from dataset.frame_cache import GpuFrameLoader
    res = {}
    for mode, resident, epochs in (("streamed", False, a.epochs_streamed),
                                   ("resident", True, a.epochs_resident)):
        loaders = {n: GpuFrameLoader(cache, a.batch, shuffle=True, resident=resident,
                                     augment=aug if n == "on" else None)
                   for n in ("off", "on")}

        def block(ld):
            def run():
                torch.cuda.synchronize()
                n, t0 = 0, time.perf_counter()
                for _ in range(epochs):
                    for b in ld:
                        n += b["image"].shape[0]
                torch.cuda.synchronize()
                return n / (time.perf_counter() - t0)
            return run
        fns = {"off": block(loaders["off"]), "on": block(loaders["on"])}
        fns["off2"] = fns["off"]
        r = {n: _stats(v, "samples_per_s") for n, v in _alternate(fns, a.rounds).items()}
        off = r["off"]["median_samples_per_s"]
        r["on"]["over_off"] = round(r["on"]["median_samples_per_s"] / off, 4)
        r["off2"]["over_off"] = round(r["off2"]["median_samples_per_s"] / off, 4)
        r["epochs_per_block"] = epochs
        res[mode] = r
        print(mode, {n: r[n]["median_samples_per_s"] for n in ("off", "on", "off2")}, flush=True)
    return res


def bench_launches(a, cache, aug):
    from dataset.frame_cache import GpuFrameLoader
    from e2ep_amd import _lib
    dev = GpuFrameLoader(cache, a.batch, resident=True).upload()
    C = cache.crop
    hw, F = C * C, a.batch * 4
    g = torch.Generator().manual_seed(0)
    idx = torch.randperm(len(cache), generator=g)[:a.batch]
    frames = (idx[:, None] * 4 + torch.arange(4)).reshape(-1).to("cuda")
    key = aug.frame_keys(idx, 4).to("cuda")
    image = torch.empty(F, 3, C, C, device="cuda")
    depth = torch.empty(F, C, C, dtype=torch.float64, device="cuda")
    sums = torch.empty(F, 3, dtype=torch.int64, device="cuda")
    mean = torch.empty(F, device="cuda")
    base = aug.base(0)
    base = base - (1 << 64) if base >> 63 else base
    p, st = _lib.ptr, _lib.stream()
    rgb, drgb = p(dev["rgb"]), p(dev["depth_rgb"])

    def plain():
        _lib.call("e2ep_decode_frames", rgb, drgb, p(frames), F, hw, p(image), p(depth), st)

    def gray():
        _lib.call("e2ep_frame_gray_mean", rgb, p(frames), F, hw, p(sums), p(mean), st)

    def jitter():
        _lib.call("e2ep_decode_frames_aug", rgb, drgb, p(frames), p(key), F, hw, p(mean), base,
                  aug.brightness, aug.contrast, aug.saturation, aug.noise, aug.gray_p, p(image),
                  p(depth), st)

    def both():
        gray()
        jitter()

    def block(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def run():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                call()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.iters * 1e3
        return run
    gray()
    fns = {"off": block(plain), "aug": block(jitter), "mean": block(gray), "on": block(both)}
    fns["off2"] = fns["off"]
    res = {n: _stats(v, "us") for n, v in _alternate(fns, a.rounds).items()}
    for n, r in res.items():
        r["model_bytes"] = BYTES[n] * F * hw
        r["gbps"] = round(r["model_bytes"] / (r["median_us"] * 1e-6) / 1e9, 1)
        r["minus_off_us"] = round(r["median_us"] - res["off"]["median_us"], 3)
    res["off_spread_us"] = round(res["off"]["max_us"] - res["off"]["min_us"], 3)
    res["config"] = f"{F} frames of {C}x{C} gathered from a resident cache, {a.iters} calls per block"
    print("launches", {n: res[n]["median_us"] for n in fns}, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7, help="timed blocks per setting")
    ap.add_argument("--epochs-streamed", type=int, default=3)
    ap.add_argument("--epochs-resident", type=int, default=30)
    ap.add_argument("--iters", type=int, default=500, help="launches per block")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from e2ep_amd import _lib
    from e2ep_amd.augment import PhotoAugment
    _lib.load()
    aug = PhotoAugment(brightness=0.4, contrast=0.4, saturation=0.4, noise=0.05, gray_p=0.1)
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "samples": a.samples,
           "crop": a.crop, "rounds": a.rounds}
    with tempfile.TemporaryDirectory() as root:
        cache = synthetic_cache(root, a.samples, a.crop)
        res["loader"] = bench_loader(a, cache, aug)
        res["launches"] = bench_launches(a, cache, aug)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
