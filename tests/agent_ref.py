"""Vectorised NumPy / torch statement of the agent's per-frame post-processing
(agent/parking_agent.py:272-318, :474-476; dataset/carla_dataset.py:90-111), used only by the
tests: the GPU kernels of csrc/agent.hip are held to it, and tests/test_agent_post_cpu.py holds
it to the recorded results of the reference (tests/golden/agent_post.json).

Also the case generators the recorder (tests/golden/make_agent_golden.py) and the tests share:
the 200 x 200 cases are stored as a RandomState seed plus a rule, not as arrays."""
import numpy as np
import torch

LUT = (0, 128, 255)
RES = (0.1, 0.1)  # bev_x_bound[2], bev_y_bound[2] of config/training.yaml


# ------------------------------------------------------------------------------------------
# case generators
# ------------------------------------------------------------------------------------------
def generate(gen):
    """Logits (C, X, Y) float32 of a generated case: {"rule": "noise_blob", "seed", "shape",
    "boost"}: standard-normal noise on every plane, plus `boost` on plane 2 inside a disc whose
    centre and radius are drawn from the same RandomState."""
    if gen["rule"] != "noise_blob":
        raise ValueError(gen["rule"])
    rs = np.random.RandomState(gen["seed"])
    C, X, Y = gen["shape"]
    a = rs.standard_normal((C, X, Y)).astype(np.float32)
    cx, cy = rs.randint(X // 5, X - X // 5), rs.randint(Y // 5, Y - Y // 5)
    rad = rs.randint(5, 20)
    r, c = np.mgrid[0:X, 0:Y]
    a[2][(r - cx) ** 2 + (c - cy) ** 2 <= rad * rad] += np.float32(gen["boost"])
    return a


_WORDS = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf}


def decode_logits(case):
    """The float32 (C, X, Y) logits of a golden case (inline values, non-finite ones as
    strings, or a generator)."""
    if "gen" in case:
        return generate(case["gen"])
    flat = [_WORDS[v] if isinstance(v, str) else v for v in case["logits"]]
    return np.asarray(flat, dtype=np.float32).reshape(case["shape"])


def encode_logits(a):
    out = []
    for v in np.asarray(a, dtype=np.float32).reshape(-1).tolist():
        out.append(v if np.isfinite(v) else ("nan" if v != v else ("inf" if v > 0 else "-inf")))
    return out


# ------------------------------------------------------------------------------------------
# the post-processing chain
# ------------------------------------------------------------------------------------------
def classes(logits):
    """Per-pixel class (X, Y) int64 of (C, X, Y) logits: torch.argmax over the planes."""
    t = torch.as_tensor(np.asarray(logits) if not torch.is_tensor(logits) else logits)
    return torch.argmax(t.detach().float().cpu(), dim=0).numpy()


def seg_image(logits, lut=LUT):
    """The display image: classes through the grey-level table, flipped top to bottom."""
    return np.asarray(lut, dtype=np.uint8)[classes(logits)][::-1].copy()


def slot(logits, res=RES, target=2):
    """The target slot of one sample: dict(found, count, tx, ty, x, y, px, py).  Rows are
    counted in the flipped image; tx, ty are the truncated integer means; (x, y) the float64
    ego-frame point (both axes offset by X / 2) and (px, py) its float32 rounding, as the
    agent's torch.tensor(target_point, dtype=torch.float) stores it.  Not found: count 0,
    tx = ty = -1 and the points None."""
    flipped = classes(logits)[::-1]
    X = flipped.shape[0]
    rows, cols = np.nonzero(flipped == target)
    n = int(rows.size)
    if n == 0:
        return dict(found=False, count=0, tx=-1, ty=-1, x=None, y=None, px=None, py=None)
    tx, ty = int(rows.sum(dtype=np.int64)) // n, int(cols.sum(dtype=np.int64)) // n
    x = np.float64(-(tx - X / 2)) * np.float64(res[0])
    y = np.float64(ty - X / 2) * np.float64(res[1])
    return dict(found=True, count=n, tx=tx, ty=ty, x=float(x), y=float(y),
                px=np.float32(x), py=np.float32(y))


def detokenize(tokens, token_nums=204):
    """(..., 3) integer tokens -> (..., 4) float64 (throttle, brake, steer, reverse 0 / 1)."""
    t = np.asarray(tokens, dtype=np.int64)
    half = np.float64((token_nums - 4) / 2)
    acc = t[..., 0] / half - 1.0
    fwd = t[..., 0] > half
    zero = np.zeros_like(acc)
    return np.stack([np.where(fwd, acc, zero), np.where(fwd, zero, -acc), t[..., 1] / half - 1.0,
                     (t[..., 2] > half).astype(np.float64)], axis=-1)


def target_used(prev, goal):
    """The target point the next predict consumes: (prev x, prev y, goal yaw) once a slot has
    been found (prev = (px, py) float32), else the goal.  float32 (3,)."""
    g = np.asarray(goal, dtype=np.float32).reshape(3)
    if prev is None:
        return g.copy()
    return np.asarray([prev[0], prev[1], g[2]], dtype=np.float32)


def bits(v):
    """The bit pattern(s) of float32 value(s), for exact comparisons that tell -0.0 from 0.0."""
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def bits64(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)
