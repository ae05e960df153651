"""Record the convolution host queries (workspace sizes, statistics tiles, weight-gradient
splits, paired-backward gate) for a list of geometries and settings into
tests/golden/conv_plans.json, through the C ABI only (no GPU call is made).

Run it on a build of the commit whose answers are to be pinned (the parent of a refactor):
    python scripts/record_conv_plans.py [--out tests/golden/conv_plans.json]
tests/test_conv_plan_cpu.py replays the file against the library under test.

dims = (N, Cin, H, W, Cout, R, S, P, Q, sh, sw, ph, pw, dh, dw).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e2e-parking-carla_amd"))

KEY_LP32, KEY_LP32W, KEY_FOLD, KEY_WGRAD_GEN, KEY_LP_WGRAD, KEY_STEM = 14, 15, 28, 9, 12, 35


def conv(n, cin, h, w, cout, k, stride=1, pad=0, dil=1):
    p = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1
    q = (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return [n, cin, h, w, cout, k, k, p, q, stride, stride, pad, pad, dil, dil]


def shapes():
    out = []
    with open(os.path.join(ROOT, "scripts", "conv_shapes.json")) as f:
        for i, e in enumerate(json.load(f)):
            out.append({"name": f"step{i:02d}", "dims": e["dims"], "grad_channels": e["grad_channels"]})

    def add(name, dims, gc=None):
        out.append({"name": name, "dims": dims, "grad_channels": gc})

    # the BEV stem at batch 4, and with output rows that are no multiple of 8 pixels
    add("stem_c4", conv(4, 65, 256, 256, 64, 7, 2, 3), 64)
    add("stem_q100", conv(4, 65, 200, 200, 64, 7, 2, 3), 64)
    add("stem_small", conv(1, 65, 32, 32, 64, 7, 2, 3), 64)
    # row-count gates (32-row tiles, k_conv_lp / k_conv_gemm2 from 40 rows): as Cout (forward)
    # and as Cin (data gradient)
    for m in (24, 32, 39, 40, 96):
        add(f"k3_cout{m}", conv(8, 64, 32, 32, m, 3, 1, 1))
        add(f"k3_cin{m}", conv(8, m, 32, 32, 64, 3, 1, 1))
        add(f"k1_cout{m}", conv(8, 64, 64, 64, m, 1))
        add(f"k1_cin{m}", conv(8, m, 64, 64, 64, 1))
    # single-step K of a 1x1 (Kc <= 32 stays on k_conv_gemm)
    for c in (32, 33):
        add(f"k1_cin{c}_to64", conv(8, c, 64, 64, 64, 1))
        add(f"k1_64_to_cout{c}", conv(8, 64, 64, 64, c, 1))
    # dead taps: dilation 24 on a 16 x 16 map keeps the centre tap only
    add("k3_dil24", conv(2, 64, 16, 16, 64, 3, 1, 24, 24))
    add("k3_dil24_n1", conv(1, 64, 16, 16, 64, 3, 1, 24, 24))
    # 1x1 maps whose pixel count is no multiple of 32 (and of 8)
    add("k1_pq100", conv(8, 64, 10, 10, 64, 1))
    add("k1_pq144", conv(8, 64, 12, 12, 64, 1))
    add("k1_pq40000", conv(8, 64, 200, 200, 3, 1))
    # k_wgrad_lp's size gate: Cout * Cin * taps = 2047 and 2048
    add("k1_2047", conv(8, 89, 16, 16, 23, 1))
    add("k1_2048", conv(8, 64, 16, 16, 32, 1))
    # the smallest shapes that reach each kernel family (tests/test_conv_gpu.py)
    add("small_k3", conv(2, 64, 16, 16, 64, 3, 1, 1))
    add("small_k1_24", conv(2, 48, 16, 16, 24, 1))
    add("small_k1_96", conv(2, 48, 16, 16, 96, 1))
    add("small_direct", conv(1, 3, 32, 32, 48, 3, 2, 0))
    return out


def settings():
    out = []
    for prec, pname in ((0, "fp32"), (1, "bf16"), (2, "fp16")):
        out.append({"name": pname, "precision": prec, "variant": 0, "tune": {}})
        for v in (1, 2, 4):
            out.append({"name": f"{pname}_variant{v}", "precision": prec, "variant": v, "tune": {}})
        for key, val in ((KEY_LP32, 2), (KEY_LP32, 1), (KEY_LP32W, 2), (KEY_FOLD, 2), (KEY_FOLD, 1),
                         (KEY_WGRAD_GEN, 1), (KEY_LP_WGRAD, 1), (KEY_STEM, 1 + 31), (KEY_STEM, 1)):
            out.append({"name": f"{pname}_key{key}_{val}", "precision": prec, "variant": 0,
                        "tune": {str(key): val}})
    # keys 14 and 15 together: the fp32 k_conv_lp / k_wgrad_lp pair
    out.append({"name": "fp32_key14_2_key15_2", "precision": 0, "variant": 0,
                "tune": {str(KEY_LP32): 2, str(KEY_LP32W): 2}})
    return out


class applied:
    """Apply one setting to the library; restore what was there on exit."""

    def __init__(self, lib, setting):
        self.lib, self.setting = lib, setting

    def __enter__(self):
        lib, s = self.lib, self.setting
        self.prec = lib.e2ep_conv_precision(s["precision"])
        self.variant = lib.e2ep_conv_gemm_variant(s["variant"])
        self.tune = [(int(k), lib.e2ep_tune(int(k), int(v))) for k, v in s["tune"].items()]

    def __exit__(self, *exc):
        lib = self.lib
        for k, v in reversed(self.tune):
            lib.e2ep_tune(k, v)
        lib.e2ep_conv_gemm_variant(self.variant)
        lib.e2ep_conv_precision(self.prec)


FIELDS = ["fwd_workspace", "dgrad_workspace", "dgrad_workspace_grad_channels", "stats_tiles_layout0",
          "stats_tiles_layout1", "wgrad_splits", "wgrad_workspace", "bwd_pair_ok",
          "bwd_pair_ok_grad_channels"]


def query(lib, shape):
    """One row of FIELDS for a shape under the library's current setting."""
    d = (ctypes.c_int * 15)(*shape["dims"])
    cin, gc = shape["dims"][1], shape["grad_channels"]
    splits = lib.e2ep_conv_wgrad_splits(d)
    return [lib.e2ep_conv_fwd_workspace(d),
            lib.e2ep_conv_dgrad_workspace(d, cin),
            lib.e2ep_conv_dgrad_workspace(d, gc) if gc else None,
            lib.e2ep_conv_fwd_stats_tiles(d, 0),
            lib.e2ep_conv_fwd_stats_tiles(d, 1),
            splits,
            lib.e2ep_conv_wgrad_workspace(d, splits),
            lib.e2ep_conv_bwd_pair_ok(d, cin),
            lib.e2ep_conv_bwd_pair_ok(d, gc) if gc else None]


BASE = {0: "fp32", 1: "bf16", 2: "fp16"}  # precision -> the setting at default tuning


def expand(gold):
    """setting name -> one row of FIELDS per shape.  The file holds every row of the three
    default-tuning settings; of any other setting only the rows (by shape index) that differ
    from its precision's default-tuning rows."""
    out = {}
    for s in gold["settings"]:
        rows = gold["results"][s["name"]]
        if isinstance(rows, dict):
            base = gold["results"][BASE[s["precision"]]]
            rows = [rows.get(str(i), b) for i, b in enumerate(base)]
        out[s["name"]] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_plans.json"))
    args = ap.parse_args()
    from e2ep_amd import _lib
    lib = _lib.load()
    shp, sets = shapes(), settings()
    results = {}
    for s in sets:
        with applied(lib, s):
            rows = [query(lib, sh) for sh in shp]
        base = results.get(BASE[s["precision"]])
        if s["name"] != BASE[s["precision"]]:
            rows = {str(i): r for i, (r, b) in enumerate(zip(rows, base)) if r != b}
        results[s["name"]] = rows
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
