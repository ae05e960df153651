"""MBConv middle A/B on the C2 step's three 16x16 shapes (N = 32 camera images): GPU time of
the chain _bn0 -> swish -> depthwise -> _bn1 -> swish -> SE (forward) and of its backward after
the SE's own gradient kernels, as the step launches it with e2ep_tune key 36 = 1 (separate
launches: e2ep_bn_stats, e2ep_dwconv_fwd_stats, e2ep_bn_stats, e2ep_se_fwd; e2ep_bn_bwd with the
SE gate, e2ep_dwconv_bwd, e2ep_bn_bwd) and = 2 (e2ep_mbconv_mid_fwd + e2ep_se_fwd_pooled;
e2ep_mbconv_mid_bwd), 20 chains in one HIP graph each.  Both forward chains include the SE MLP
and excite, which the fused kernel does not replace; the fused launches are also timed alone and
set against their HBM floor (forward 2 tensors, backward 4) at --peak TB/s.

    python scripts/bench_mbconv_mid.py [--peak 8.0]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "e2e-parking-carla_amd"), ROOT, os.path.join(ROOT, "scripts")]
import torch  # noqa: E402

from bench_gemm import timed  # noqa: E402

# (C, K, layers) of the EfficientNet-B4 trunk's 16x16 stride-1 blocks (bench_dw.py SHAPES)
SHAPES = [(672, 3, 5), (672, 5, 1), (960, 5, 5)]
N, H = 32, 16
EPS, MOM = 1e-3, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peak", type=float, default=8.0, help="HBM peak, TB/s")
    args = ap.parse_args()
    from e2ep_amd import _lib
    lib = _lib.load()
    p, s = _lib.ptr, _lib.stream
    f = dict(device="cuda", dtype=torch.float32)
    tot = {}
    for C, K, layers in SHAPES:
        sq = C // 24
        d = _lib.dims((N, C, H, H, K, H, H, 1, K // 2, K // 2))
        y0, gy = torch.randn(N, C, H, H, **f), torch.randn(N, C, H, H, **f)
        w = torch.randn(C, 1, K, K, **f) / K
        g0, b0, g1, b1 = (torch.randn(C, **f) * 0.1 + o for o in (1, 0, 1, 0))
        rm0, rv0, rm1, rv1 = (torch.zeros(C, **f) for _ in range(4))
        st0, st1 = torch.empty(4, C, **f), torch.empty(4, C, **f)
        y1, y, dt, dy1, dx = (torch.empty_like(y0) for _ in range(5))
        pooled, a = torch.empty(N, C, **f), torch.empty(N, C, **f)
        hpre = torch.empty(N, sq, **f)
        w1, sb1 = torch.randn(sq, C, **f) / C ** 0.5, torch.zeros(sq, **f)
        w2, sb2 = torch.randn(C, sq, **f) / sq ** 0.5, torch.zeros(C, **f)
        dpooled = torch.randn(N, C, **f) * 0.01
        dg0, db0, dg1, db1 = (torch.empty(C, **f) for _ in range(4))
        dw = torch.empty_like(w)
        ws = torch.empty(max(lib.e2ep_bn_workspace(N, C, H, H), 16), dtype=torch.uint8, device="cuda")
        wsw = torch.empty(max(lib.e2ep_dwconv_wgrad_workspace(d), 16), dtype=torch.uint8, device="cuda")

        def bn_stats(x, g, b, rm, rv, st):
            _lib.call("e2ep_bn_stats", p(x), p(g), p(b), p(rm), p(rv), N, C, H, H, 1, MOM, EPS,
                      p(st[0]), p(st[1]), p(st[2]), p(st[3]), p(ws), _lib.nbytes(ws), s(), 0)

        def se(name):
            _lib.call(name, p(y1), p(st1[2]), p(st1[3]), p(w1), p(sb1), p(w2), p(sb2), N, C, H * H,
                      sq, p(pooled), p(hpre), p(a), p(y), s(), 0)

        def fwd_sep():
            bn_stats(y0, g0, b0, rm0, rv0, st0)
            _lib.call("e2ep_dwconv_fwd_stats", p(y0), p(w), d, p(st0[2]), p(st0[3]), 2, p(y1), None,
                      0, s(), 0)
            bn_stats(y1, g1, b1, rm1, rv1, st1)
            se("e2ep_se_fwd")

        def mid_fwd():
            _lib.call("e2ep_mbconv_mid_fwd", p(y0), p(w), d, p(g0), p(b0), p(rm0), p(rv0), MOM, EPS,
                      p(st0), p(g1), p(b1), p(rm1), p(rv1), MOM, EPS, p(st1), p(y1), p(pooled), s())

        def fwd_fused():
            mid_fwd()
            se("e2ep_se_fwd_pooled")

        def bn_bwd(x, dy, st, g, b, gate, out, dg, db):
            _lib.call("e2ep_bn_bwd", p(x), p(dy), p(st[0]), p(st[1]), p(g), p(b), None, None, 1.0,
                      p(a) if gate else None, p(dpooled) if gate else None, N, C, H, H, 1, 2, p(out),
                      p(dg), p(db), None, p(ws), _lib.nbytes(ws), s(), 0)

        def bwd_sep():
            bn_bwd(y1, gy, st1, g1, b1, True, dy1, dg1, db1)
            _lib.call("e2ep_dwconv_bwd", p(dy1), p(y0), p(w), d, p(st0[2]), p(st0[3]), 2, p(dt),
                      p(wsw), _lib.nbytes(wsw), p(dw), s(), 0)
            bn_bwd(y0, dt, st0, g0, b0, False, dx, dg0, db0)

        def bwd_fused():
            _lib.call("e2ep_mbconv_mid_bwd", p(gy), p(a), p(dpooled), p(y1), p(y0), p(w), d, p(st1),
                      p(g1), p(b1), p(st0), p(g0), p(b0), p(dx), p(dg1), p(db1), p(dg0), p(db0),
                      p(dw), s())

        prev = lib.e2ep_tune(36, 2)
        try:
            us = {"fwd key1": timed(fwd_sep, 20), "fwd key2": timed(fwd_fused, 20),
                  "bwd key1": timed(bwd_sep, 20), "bwd key2": timed(bwd_fused, 20),
                  "mid_fwd": timed(mid_fwd, 20)}
        finally:
            lib.e2ep_tune(36, prev)
        mb = 4.0 * N * C * H * H / 1e6  # one tensor
        floor_f, floor_b = 2 * mb / args.peak, 4 * mb / args.peak
        print(f"C{C:4d} k{K} x{layers}: " + " ".join(f"{k} {v:6.1f} us" for k, v in us.items())
              + f" | k_mbconv_mid_fwd {2 * mb / us['mid_fwd']:.2f} TB/s = {floor_f / us['mid_fwd']:.0%} of "
              f"the {floor_f:.1f} us floor, k_mbconv_mid_bwd {4 * mb / us['bwd key2']:.2f} TB/s = "
              f"{floor_b / us['bwd key2']:.0%} of the {floor_b:.1f} us floor", flush=True)
        for k, v in us.items():
            tot[k] = tot.get(k, 0.0) + layers * v
    print("step total us: " + " ".join(f"{k} {v:.0f}" for k, v in tot.items()), flush=True)
    print(f"saved per step: forward {tot['fwd key1'] - tot['fwd key2']:.0f} us, backward "
          f"{tot['bwd key1'] - tot['bwd key2']:.0f} us", flush=True)


if __name__ == "__main__":
    main()
