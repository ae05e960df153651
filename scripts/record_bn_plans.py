"""Record the BatchNorm host queries (split workspace, forward / backward single-launch gates)
and the fused MBConv middle's gate for a list of shapes and settings into
tests/golden/bn_plans.json, through the C ABI only (no GPU call is made).

Run it on a build of the commit whose answers are to be pinned (the parent of a refactor):
    python scripts/record_bn_plans.py [--out tests/golden/bn_plans.json]
tests/test_bn_plan_cpu.py replays the file against the library under test.

A shape is (N, C, H, W) of the BatchNorm's input.  e2ep_mbconv_mid_ok is asked for the 16 x 16,
stride-1, SAME depthwise geometry with the shape's N and C, K = 3 and K = 5 (whatever the
shape's own H and W: the fused middle's BatchNorm channels hold N * 64 float4).  Degenerate
shapes (N, C, H or W <= 0) are asked the two split queries only.

The model's shapes: every BatchNorm follows a convolution, so they are the distinct (Cout, P, Q)
of scripts/conv_shapes.json (dims = N, Cin, H, W, Cout, R, S, P, Q, ...) and the distinct
(C, ceil(H / stride), ceil(H / stride)) of scripts/bench_dw.py's SHAPES (C, H, K, stride, count),
each at N = 8 and N = 32 (the two image counts conv_shapes.json itself holds: 8 BEV maps, 32
camera images).
"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e2e-parking-carla_amd"))

KEY_SPLIT_TARGET, KEY_SPLIT_MIN, KEY_WIDE, KEY_WIDE_LO, KEY_MID = 0, 1, 25, 26, 36
BNS_MAX = 2048  # e2ep_bn_small_limits' default and clamp (float4 per channel)

# tests/test_nn_ops_gpu.py::test_bn_act, ::test_bn_drop_connect_fused and
# tests/test_bf16_store_gpu.py::test_bn_bwd_bf16_io_bitwise (tests/test_bn_plan_cpu.py holds the
# files to each other)
TEST_BN_ACT = [(4, 24, 32, 32), (3, 7, 5, 9), (32, 6, 1, 1), (4, 160, 8, 8), (16, 128, 32, 32),
               (8, 16, 64, 64), (3, 12, 44, 36), (2, 8, 136, 128), (32, 24, 16, 16)]
TEST_BN_DROP_CONNECT = [(8, 24, 16, 16), (6, 10, 5, 7), (16, 136, 8, 8)]
TEST_BN_BWD_BF16 = [(32, 672, 16, 16), (8, 336, 32, 32), (8, 192, 64, 64), (32, 144, 64, 64)]
# channels of 256 / 257, 512 / 513, 1024 / 1025, 2048 / 2049 float4: one vector either side of
# each single-launch layout switch (tests/test_nn_ops_gpu.py::test_bn_act_layouts runs them)
LAYOUT_BOUNDARIES = [(4, 3, 16, 16), (257, 3, 2, 2), (8, 3, 16, 16), (27, 3, 19, 4),
                     (16, 3, 16, 16), (25, 3, 41, 4), (32, 3, 16, 16), (3, 3, 683, 4)]


def model_shapes():
    """Distinct (C, P, Q) of the model's convolution and depthwise outputs, in file order."""
    out = []
    with open(os.path.join(ROOT, "scripts", "conv_shapes.json")) as f:
        for e in json.load(f):
            out.append((e["dims"][4], e["dims"][7], e["dims"][8]))
    spec = importlib.util.spec_from_file_location("bench_dw", os.path.join(ROOT, "scripts", "bench_dw.py"))
    bench_dw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench_dw)
    for C, H, _, st, _ in bench_dw.SHAPES:
        out.append((C, (H + st - 1) // st, (H + st - 1) // st))
    return list(dict.fromkeys(out))


def shapes():
    out = []

    def add(name, shape):
        out.append({"name": name, "shape": list(shape)})

    for n in (32, 8):
        for C, P, Q in model_shapes():
            add(f"model_n{n}_c{C}_{P}x{Q}", (n, C, P, Q))
    for i, s in enumerate(TEST_BN_ACT):
        add(f"test_bn_act{i:02d}", s)
    for i, s in enumerate(TEST_BN_DROP_CONNECT):
        add(f"test_bn_drop_connect{i:02d}", s)
    for i, s in enumerate(TEST_BN_BWD_BF16):
        add(f"test_bn_bwd_bf16_{i:02d}", s)
    for s in LAYOUT_BOUNDARIES:
        add(f"totv{s[0] * s[2] * s[3] // 4}", s)
    add("hw_not_mult4", (3, 7, 5, 9))
    add("per_c_below_key1", (2, 4, 8, 8))       # cap 0 -> 1 split
    add("cap_256_splits", (32, 1, 256, 256))
    add("want_1", (8, 8192, 8, 8))
    add("c65535", (1, 65535, 2, 2))
    add("degenerate_n0", (0, 8, 16, 16))
    add("degenerate_c0", (8, 0, 16, 16))
    add("degenerate_h-1", (8, 8, -1, 16))
    return out


def settings():
    def tune(name, **kv):
        return {"name": name, "tune": {k[1:]: v for k, v in kv.items()}, "bn_small": None, "limits": None}

    return [tune("default"),
            dict(tune("bn_small_0"), bn_small=0),
            dict(tune("limits_1024_1024"), limits=[1024, 1024]),
            dict(tune("limits_0_2048"), limits=[0, 2048]),
            tune("key0_2048", k0=2048), tune("key0_32768", k0=32768),
            tune("key1_1024", k1=1024), tune("key1_16384", k1=16384),
            tune("key25_1", k25=1), tune("key26_2", k26=2), tune("key25_1_key26_2", k25=1, k26=2),
            tune("key36_1", k36=1)]


class applied:
    """Apply one setting to the library; restore what was there on exit (the limits, which
    cannot be read back, to their default)."""

    def __init__(self, lib, setting):
        self.lib, self.setting = lib, setting

    def __enter__(self):
        s = self.setting
        self.tune = [(int(k), self.lib.e2ep_tune(int(k), int(v))) for k, v in s["tune"].items()]
        self.small = self.lib.e2ep_bn_small(s["bn_small"]) if s["bn_small"] is not None else None
        if s["limits"]:
            self.lib.e2ep_bn_small_limits(*s["limits"])

    def __exit__(self, *exc):
        if self.setting["limits"]:
            self.lib.e2ep_bn_small_limits(BNS_MAX, BNS_MAX)
        if self.small is not None:
            self.lib.e2ep_bn_small(self.small)
        for k, v in reversed(self.tune):
            self.lib.e2ep_tune(k, v)


FIELDS = ["workspace", "fwd_split", "bwd_split", "mid_ok_k3", "mid_ok_k5"]


def mid_dims(N, C, K):
    """dims[10] of the fused middle's depthwise conv: 16 x 16, stride 1, SAME."""
    return [N, C, 16, 16, K, 16, 16, 1, (K - 1) // 2, (K - 1) // 2]


def query(lib, shape):
    """One row of FIELDS for a shape under the library's current setting (None: not asked)."""
    N, C, H, W = shape
    split = [lib.e2ep_bn_fwd_split(N, C, H, W), lib.e2ep_bn_bwd_split(N, C, H, W)]
    if min(shape) <= 0:
        return [None, *split, None, None]
    mid = [lib.e2ep_mbconv_mid_ok((ctypes.c_int * 10)(*mid_dims(N, C, K))) for K in (3, 5)]
    return [lib.e2ep_bn_workspace(N, C, H, W), *split, *mid]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bn_plans.json"))
    args = ap.parse_args()
    from e2ep_amd import _lib
    lib = _lib.load()
    shp, sets = shapes(), settings()
    results = {}
    for s in sets:
        with applied(lib, s):
            results[s["name"]] = [query(lib, sh["shape"]) for sh in shp]
    with open(args.out, "w") as f:
        f.write('{\n"fields": %s,\n"shapes": [\n' % json.dumps(FIELDS))
        f.write(",\n".join(json.dumps(sh) for sh in shp))
        f.write('\n],\n"settings": [\n')
        f.write(",\n".join(json.dumps(s) for s in sets))
        f.write('\n],\n"results": {\n')
        f.write(",\n".join('"%s": %s' % (s["name"], json.dumps(results[s["name"]], separators=(",", ":")))
                           for s in sets))
        f.write("\n}\n}\n")
    print(f"{len(shp)} shapes x {len(sets)} settings -> {args.out}")


if __name__ == "__main__":
    main()
