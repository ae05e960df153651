"""Generate tests/golden/depth_cells.npz by running the REFERENCE's own
DepthLoss.get_down_sampled_gt_depth (loss/depth_loss.py) on a small planted depth tensor.

Run in the build container only (needs /root/reference):
    python tests/golden/make_depth_golden.py

loss/depth_loss.py and tool/config.py are imported unmodified, with the reference's own
config/training.yaml (d_bound, bev_down_sample).  No reference source is copied: only the
planted input and the recorded one-hot labels are written.  The input is a (2, 3, 16, 24)
depth tensor, six 8 x 8 cells per image, seeded uniform metres with these cells planted:
    all zeros (read as 1e5: background)          a minimum of exactly 0.25 (bin 0: background)
    a minimum of exactly 0.5 (the first bin)     12.49 (the last bin)
    exactly 12.5 (D + 1: out of range)           all 1e5
    one small value among zeros                  0.75 - 1e-10, which is 0.75 as float32: the
                                                 float64 labels and the float32 labels differ
It is recorded once as float64 and once rounded to float32, with the reference's labels of
each.  Before writing, the script asserts that tests/depth_ref.py gives the same labels."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "depth_cells.npz")
sys.path.insert(0, os.path.join(REPO, "tests"))

import depth_ref  # noqa: E402

DOWN = 8


def planted():
    rng = np.random.RandomState(20)
    d = rng.uniform(0.3, 14.0, (2, 3, 16, 24))

    def cell(b, n, i, j):
        return d[b, n, i * DOWN:(i + 1) * DOWN, j * DOWN:(j + 1) * DOWN]

    cell(0, 0, 0, 0)[:] = 0.0
    c = cell(0, 0, 0, 1)
    c[:] = np.maximum(c, 1.0)
    c[3, 5] = 0.25
    c = cell(0, 1, 1, 0)
    c[:] = np.maximum(c, 1.0)
    c[0, 0] = 0.5
    c = cell(0, 2, 1, 2)
    c[:] = 13.0
    c[7, 7] = 12.49
    cell(1, 0, 0, 2)[:] = 12.5
    cell(1, 1, 0, 0)[:] = 1e5
    c = cell(1, 2, 1, 1)
    c[:] = 0.0
    c[4, 4] = 0.7
    c = cell(1, 2, 0, 0)
    c[:] = 3.0
    c[2, 6] = 0.75 - 1e-10
    return d


def main():
    import yaml
    sys.path.insert(0, REF)
    from loss.depth_loss import DepthLoss
    from tool.config import get_cfg
    assert os.path.abspath(sys.modules["loss.depth_loss"].__file__).startswith(REF)

    with open(os.path.join(REF, "config", "training.yaml")) as f:
        cfg = get_cfg(yaml.safe_load(f))
    assert cfg.bev_down_sample == DOWN
    loss = DepthLoss(cfg)
    D = loss.depth_channels
    d64 = planted()
    d32 = d64.astype(np.float32)
    out = {"d_bound": np.asarray(cfg.d_bound, dtype=np.float64), "down": np.int64(DOWN),
           "depth_f64": d64, "depth_f32": d32}
    for name, d in (("f64", d64), ("f32", d32)):
        onehot = loss.get_down_sampled_gt_depth(torch.from_numpy(d)).numpy()
        assert onehot.shape == (2 * 3 * 2 * 3, D) and set(np.unique(onehot)) <= {0.0, 1.0}
        out["onehot_" + name] = onehot.astype(np.uint8)
        k, _ = depth_ref.classes(d.reshape(6, 16, 24), cfg.d_bound, DOWN)
        ref = np.eye(D + 1, dtype=np.uint8)[k.reshape(-1)][:, 1:]
        assert np.array_equal(ref, out["onehot_" + name]), name
        print(name, "classes", k.reshape(6, -1).tolist())
    assert not np.array_equal(out["onehot_f64"], out["onehot_f32"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
