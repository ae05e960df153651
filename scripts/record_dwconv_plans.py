"""Record the depthwise-convolution host queries (statistics tiles, paired-backward gate, bf16
storage gate, weight-gradient workspace) for a list of geometries and settings into
tests/golden/dwconv_plans.json, through the C ABI only (no GPU call is made).

Run it on a build of the commit whose answers are to be pinned (the parent of a refactor):
    python scripts/record_dwconv_plans.py [--out tests/golden/dwconv_plans.json]
tests/test_dwconv_plan_cpu.py replays the file against the library under test.

A case is (N, C, H, W, K, stride, (pad_left, pad_right, pad_top, pad_bottom)), as in
tests/test_nn_ops_gpu.py; dims = (N, C, H, W, K, P, Q, stride, pad_top, pad_left).
"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e2e-parking-carla_amd"))

KEY_WGRAD_TARGET, KEY_VEC = 3, 23

# tests/test_nn_ops_gpu.py::test_depthwise (before the halo cases) and
# ::test_depthwise_bwd_pair_bitwise_equals_two_launches (tests/test_dwconv_plan_cpu.py holds the
# two files to each other)
TEST_DEPTHWISE = [
    (4, 144, 64, 64, 3, 2, (0, 1, 0, 1)), (4, 48, 32, 32, 3, 1, (1, 1, 1, 1)),
    (4, 192, 32, 32, 5, 2, (2, 2, 2, 2)), (2, 672, 16, 16, 5, 1, (2, 2, 2, 2)),
    (3, 8, 13, 11, 3, 2, (0, 1, 0, 1)), (2, 24, 128, 128, 3, 1, (1, 1, 1, 1)),
    (2, 8, 128, 128, 3, 2, (0, 1, 0, 1)), (2, 32, 64, 64, 3, 1, (1, 1, 1, 1)),
    (2, 40, 32, 32, 5, 1, (2, 2, 2, 2)), (3, 16, 16, 16, 3, 1, (1, 1, 1, 1)),
    (2, 12, 24, 20, 5, 1, (2, 2, 2, 2)), (2, 16, 32, 32, 5, 2, (1, 2, 1, 2)),
    (2, 8, 20, 24, 3, 2, (0, 1, 0, 1)), (2, 6, 64, 48, 5, 2, (2, 2, 2, 2)),
    (2, 16, 32, 32, 5, 1, (3, 1, 3, 1))]
TEST_BWD_PAIR = [
    (4, 48, 32, 32, 3, 1, (1, 1, 1, 1)), (2, 672, 16, 16, 5, 1, (2, 2, 2, 2)),
    (2, 24, 128, 128, 3, 1, (1, 1, 1, 1)), (2, 32, 64, 64, 3, 1, (1, 1, 1, 1)),
    (2, 40, 32, 32, 5, 1, (2, 2, 2, 2)), (3, 16, 16, 16, 3, 1, (1, 1, 1, 1)),
    (2, 12, 24, 20, 5, 1, (2, 2, 2, 2)), (32, 192, 32, 32, 5, 1, (2, 2, 2, 2)),
    (32, 96, 64, 64, 3, 1, (1, 1, 1, 1)), (4, 144, 64, 64, 3, 2, (0, 1, 0, 1)),
    (2, 16, 32, 32, 3, 2, (1, 1, 1, 1)), (4, 192, 32, 32, 5, 2, (2, 2, 2, 2)),
    (2, 16, 32, 32, 5, 2, (1, 2, 1, 2)), (8, 144, 128, 128, 3, 2, (0, 1, 0, 1)),
    (2, 6, 64, 48, 5, 2, (2, 2, 2, 2))]


def dims_of(case):
    N, C, H, W, K, s, (l, r, t, b) = case
    return [N, C, H, W, K, (H + t + b - K) // s + 1, (W + l + r - K) // s + 1, s, t, l]


def shapes():
    out = []

    def add(name, case):
        out.append({"name": name, "case": [*case[:6], list(case[6])], "dims": dims_of(case)})

    spec = importlib.util.spec_from_file_location("bench_dw", os.path.join(ROOT, "scripts", "bench_dw.py"))
    bench_dw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench_dw)
    for n in (32, 8):  # the trunk at the benchmark's batch and at a quarter of it
        for C, H, K, st, _ in bench_dw.SHAPES:
            add(f"trunk_n{n}_c{C}_h{H}_k{K}_s{st}", (n, C, H, H, K, st, bench_dw.pads(H, K, st)))
    for i, c in enumerate(TEST_DEPTHWISE):
        add(f"test_depthwise{i:02d}", c)
    for i, c in enumerate(TEST_BWD_PAIR):
        add(f"test_bwd_pair{i:02d}", c)
    # W or Q no multiple of 4
    add("w11_q11_s1", (2, 8, 13, 11, 3, 1, (1, 1, 1, 1)))
    add("w12_q11_s1", (2, 8, 13, 12, 3, 1, (1, 0, 1, 1)))
    # Q = 256 / 260 (a unit is one 256-wide row at most)
    add("q256_s1", (1, 4, 16, 256, 3, 1, (1, 1, 1, 1)))
    add("q260_s1", (1, 4, 16, 260, 3, 1, (1, 1, 1, 1)))
    add("q256_s2", (1, 4, 16, 512, 3, 2, (0, 1, 0, 1)))
    add("q260_s2", (1, 4, 16, 520, 3, 2, (0, 1, 0, 1)))
    # the staging's reach IR * W / 4 <= 384 float4: K 3 / s 2 / W 256 is 320, K 5 is 448
    add("reach_k3_s2_w256", (2, 8, 256, 256, 3, 2, (0, 1, 0, 1)))
    add("reach_k5_s2_w256", (2, 8, 256, 256, 5, 2, (1, 2, 1, 2)))
    add("reach_k5_s1_w256", (2, 8, 256, 256, 5, 1, (2, 2, 2, 2)))
    # DW_S2_PAIR_UNITS = 131072 data-gradient units: 14 * 144 * 64 = 129024, 15 -> 138240
    add("s2_pair_units_n14", (14, 144, 128, 128, 3, 2, (0, 1, 0, 1)))
    add("s2_pair_units_n15", (15, 144, 128, 128, 3, 2, (0, 1, 0, 1)))
    # stride 2, pad_left 0 .. 3
    for K, pads in ((3, ((0, 1), (1, 1), (2, 0), (3, 0))), (5, ((0, 3), (1, 2), (2, 2), (3, 1)))):
        for l, r in pads:
            add(f"s2_k{K}_pl{l}", (2, 16, 32, 32, K, 2, (l, r, l, r)))
    # stride 1, asymmetric pads (the flipped data-gradient geometry has pad_left K - 1 - pad_left)
    add("s1_k5_pad3131_n4", (4, 24, 32, 32, 5, 1, (3, 1, 3, 1)))
    add("s1_k5_pad4040", (2, 16, 32, 32, 5, 1, (4, 0, 4, 0)))
    add("s1_k5_pad0404", (2, 16, 32, 32, 5, 1, (0, 4, 0, 4)))
    add("s1_k3_pad2020", (2, 16, 32, 32, 3, 1, (2, 0, 2, 0)))
    add("s1_k3_pad0202", (2, 16, 32, 32, 3, 1, (0, 2, 0, 2)))
    # N = 1: the split cap (8 units, or 2048 pixels, per split)
    add("n1_c48_h32", (1, 48, 32, 32, 3, 1, (1, 1, 1, 1)))
    add("n1_c672_h16", (1, 672, 16, 16, 5, 1, (2, 2, 2, 2)))
    add("n1_c8_13x11", (1, 8, 13, 11, 3, 2, (0, 1, 0, 1)))
    # filters / strides without a kernel
    add("k7", (2, 8, 32, 32, 7, 1, (3, 3, 3, 3)))
    add("s3", (2, 8, 32, 32, 3, 3, (1, 1, 1, 1)))
    return out


def settings():
    return [{"name": "default", "tune": {}},
            {"name": "key23_1", "tune": {str(KEY_VEC): 1}},
            {"name": "key3_64", "tune": {str(KEY_WGRAD_TARGET): 64}},
            {"name": "key3_2048", "tune": {str(KEY_WGRAD_TARGET): 2048}}]


class applied:
    """Apply one setting to the library; restore what was there on exit."""

    def __init__(self, lib, setting):
        self.lib, self.setting = lib, setting

    def __enter__(self):
        self.tune = [(int(k), self.lib.e2ep_tune(int(k), int(v))) for k, v in self.setting["tune"].items()]

    def __exit__(self, *exc):
        for k, v in reversed(self.tune):
            self.lib.e2ep_tune(k, v)


FIELDS = ["stats_tiles", "bwd_pair_ok", "bf16_ok", "wgrad_workspace"]


def query(lib, dims):
    """One row of FIELDS for dims under the library's current setting."""
    d = (ctypes.c_int * 10)(*dims)
    return [lib.e2ep_dwconv_fwd_stats_tiles(d), lib.e2ep_dwconv_bwd_pair_ok(d),
            lib.e2ep_dwconv_bf16_ok(d), lib.e2ep_dwconv_wgrad_workspace(d)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dwconv_plans.json"))
    args = ap.parse_args()
    from e2ep_amd import _lib
    lib = _lib.load()
    shp, sets = shapes(), settings()
    results = {}
    for s in sets:
        with applied(lib, s):
            results[s["name"]] = [query(lib, sh["dims"]) for sh in shp]
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
