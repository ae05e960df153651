"""Record the GEMM host queries (e2ep_gemm_workspace, e2ep_gemm_rowsum_workspace) for a list of
shapes and settings into tests/golden/gemm_plans.json, through the C ABI only (no GPU call is
made).

Run it on a build of the commit whose answers are to be pinned (the parent of a refactor):
    python scripts/record_gemm_plans.py [--out tests/golden/gemm_plans.json]
tests/test_gemm_plan_cpu.py replays the file against the library under test.

A shape is (M, N, K) of C[M][N] = A[M][K] B[K][N]; both queries are asked for every shape.

The model's shapes: the forward rows (both operands k-contiguous) of scripts/bench_gemm.py's ROWS,
which are the linears of one B = 8 step (2048 encoder rows, 112 decoder rows), and the same with
the rows divided by 8 (B = 1: 256 and 14 rows); each as the forward (M, N, K), the input
gradient (M, K, N) and the weight gradient (N, K, M).
"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e2e-parking-carla_amd"))

KEY_SPLIT_TARGET, KEY_FOLD = 4, 28
SPLITS_ABOVE_KSTEPS = 1000  # more than the K-steps (32 deep) of any K listed here

# tests/test_gemm_gpu.py: SHAPES, test_gemm_epilogue_bias_add_relu, test_gemm_bf16_operands_vs_
# rounded_fp64 as (M, N, K); test_gemm_rowsum_weight_and_bias_gradient as (rows, N, K), asked as
# the product (N, K, rows); PAIR_SHAPES as the linear's (rows M, out N, in K), asked as its two
# gradients (tests/test_gemm_plan_cpu.py holds the files to each other)
TEST_SHAPES = [(2048, 774, 258), (2048, 258, 2048), (258, 2048, 2048), (774, 258, 2048),
               (112, 516, 258), (112, 204, 258), (8, 64, 3), (8, 256, 128), (1, 1, 1), (65, 130, 17),
               (3, 5, 700), (200, 3, 64), (14, 2048, 258), (16, 258, 2048), (14, 205, 258)]
TEST_EPILOGUE = [(2048, 258, 258), (112, 204, 258), (37, 70, 2048), (14, 2048, 258), (15, 258, 2048),
                 (7, 33, 17)]
TEST_ROWSUM = [(2048, 774, 258), (2048, 258, 2048), (2048, 2048, 258), (112, 258, 258),
               (112, 204, 258), (24, 64, 15), (37, 70, 100), (5, 3, 32), (300, 33, 64)]
TEST_BF16 = [(2048, 774, 258), (258, 2048, 2048), (112, 516, 258), (65, 130, 17), (2048, 258, 2048)]
TEST_PAIR = [(112, 258, 258), (112, 774, 258), (112, 2048, 258), (112, 258, 2048),
             (2048, 258, 258), (2048, 2048, 258), (97, 130, 333), (33, 64, 1500)]
TEST_FORCED = [(197, 301, 333), (197, 256, 333), (197, 301, 777)]  # the every-tile tests, the short workspace

# the 32 x 128 tile is taken when M mod 64 is in 1..32
TILE_M = [31, 32, 33, 64, 65, 96, 97, 112, 128]
# 63 and 64 blocks of 64 x 64: below 64 the split cap is 16, not 8, and e2ep_gemm_split_min applies
GRID_MN = [(448, 576), (512, 512)]
# a ragged last K-step; K-steps / minimum crossing 1, 2 and 8
EDGE_K = [32, 33, 255, 256, 257, 511, 512, 2048, 4096]


def model_linears():
    """(name, rows, out, in) of the model's linears at B = 8, in file order."""
    spec = importlib.util.spec_from_file_location("bench_gemm", os.path.join(ROOT, "scripts", "bench_gemm.py"))
    bench_gemm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench_gemm)
    return [(name, M, N, K) for name, M, N, K, ak, bk, _ in bench_gemm.ROWS if ak and bk]


def linear_products(M, N, K):
    """The three products of a linear with M rows, N outputs, K inputs."""
    return [("fwd", (M, N, K)), ("dgrad", (M, K, N)), ("wgrad", (N, K, M))]


def shapes():
    out = []

    def add(name, shape):
        out.append({"name": name, "shape": list(shape)})

    for batch in (8, 1):
        for name, M, N, K in model_linears():
            for kind, s in linear_products(M * batch // 8, N, K):
                add(f"model_b{batch}_{name.rsplit(' ', 1)[0].replace(' ', '_')}_{kind}", s)
    for label, lst in (("test_shapes", TEST_SHAPES), ("test_epilogue", TEST_EPILOGUE),
                       ("test_bf16_", TEST_BF16), ("test_forced", TEST_FORCED)):
        for i, s in enumerate(lst):
            add(f"{label}{i:02d}", s)
    for i, (rows, N, K) in enumerate(TEST_ROWSUM):
        add(f"test_rowsum{i:02d}", (N, K, rows))
    for i, s in enumerate(TEST_PAIR):
        for kind, p in linear_products(*s)[1:]:
            add(f"test_pair{i:02d}_{kind}", p)
    for M in TILE_M:
        add(f"tile_m{M}", (M, 258, 258))
    for M, N in GRID_MN:
        for K in EDGE_K:
            add(f"grid{M}x{N}_k{K}", (M, N, K))
    for K in EDGE_K:
        add(f"rows112_k{K}", (112, 258, K))
    add("degenerate_m0", (0, 258, 258))
    add("degenerate_n0", (112, 0, 258))
    add("degenerate_k-1", (112, 258, -1))
    return out


def settings(lib):
    """The settings to record.  e2ep_tune key 4's two values are half and twice the library's
    default, read back through e2ep_tune."""
    def s(name, **kv):
        base = {"name": name, "force": None, "split_min": None, "tune": {}, "precision": None, "skinny": None}
        base.update(kv)
        return base

    target = lib.e2ep_tune(KEY_SPLIT_TARGET, 0)
    out = [s("default")]
    for t in range(1, 7):
        for sp in (1, 3, SPLITS_ABOVE_KSTEPS):
            out.append(s(f"force_t{t}_s{sp}", force=[t, sp]))
    out += [s(f"split_min_{m}", split_min=m) for m in (1, 2, 4)]
    out += [s("key4_half", tune={str(KEY_SPLIT_TARGET): target // 2}),
            s("key4_twice", tune={str(KEY_SPLIT_TARGET): target * 2})]
    # the three below are expected to change no answer: recording them pins exactly that
    out += [s("precision_1", precision=1), s("key28_1", tune={str(KEY_FOLD): 1}),
            s("key28_2", tune={str(KEY_FOLD): 2}), s("skinny_0", skinny=0), s("skinny_128", skinny=128)]
    return out


class applied:
    """Apply one setting to the library; restore what was there on exit (the forced plan, which
    cannot be read back, to automatic)."""

    def __init__(self, lib, setting):
        self.lib, self.setting = lib, setting

    def __enter__(self):
        s, lib = self.setting, self.lib
        self.tune = [(int(k), lib.e2ep_tune(int(k), int(v))) for k, v in s["tune"].items()]
        self.split_min = lib.e2ep_gemm_split_min(s["split_min"]) if s["split_min"] is not None else None
        self.precision = lib.e2ep_gemm_precision(s["precision"]) if s["precision"] is not None else None
        self.skinny = lib.e2ep_gemm_skinny(s["skinny"]) if s["skinny"] is not None else None
        if s["force"]:
            lib.e2ep_gemm_force(*s["force"], 0)

    def __exit__(self, *exc):
        lib = self.lib
        if self.setting["force"]:
            lib.e2ep_gemm_force(0, 0, 0)
        if self.skinny is not None:
            lib.e2ep_gemm_skinny(self.skinny)
        if self.precision is not None:
            lib.e2ep_gemm_precision(self.precision)
        if self.split_min is not None:
            lib.e2ep_gemm_split_min(self.split_min)
        for k, v in reversed(self.tune):
            lib.e2ep_tune(k, v)


FIELDS = ["workspace", "rowsum_workspace"]


def query(lib, shape):
    """One row of FIELDS for a shape under the library's current setting."""
    return [lib.e2ep_gemm_workspace(*shape), lib.e2ep_gemm_rowsum_workspace(*shape)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gemm_plans.json"))
    args = ap.parse_args()
    from e2ep_amd import _lib
    lib = _lib.load()
    shp, sets = shapes(), settings(lib)
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
