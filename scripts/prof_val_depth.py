"""Workload for a kernel trace of the depth metrics beside the depth loss: an eager
ValStep(depth_metrics=True) (ParkingModel, B = 8, 4 x 256^2, fp32), `--calls` calls after the
constructor's warm-up, so every call launches k_depth_bce_fwd and the two k_depth_metrics
kernels once on the same pred_depth and depth.  Run it under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python scripts/prof_val_depth.py --calls 20

and read the three kernels' rows of OUT/**/run_kernel_stats.csv (profiles/depth_metrics/)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "e2e-parking-carla_amd"), ROOT]
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
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
    val = ValStep(mod, data, noise=noise, graph=False, depth_metrics=True)
    for _ in range(a.calls):
        val()
    r = val.result()
    print({k: v for k, v in r.items() if k.startswith("depth_") and k != "depth_per_camera"},
          "batches", r["batches"])


if __name__ == "__main__":
    main()
