// Internal interface shared by the convolution kernel files (conv.hip, conv_lp.hip,
// conv_stem.hip).
#pragma once
#include <type_traits>

#include "common.h"

namespace e2ep {

constexpr int MAXTAPS = 64;  // live filter taps per phase (R * S <= 64)

struct ConvGeom {
  int N;            // images
  int Cin, H, W;    // input
  int Cout, R, S;   // filter
  int P, Q;         // output spatial
  int sh, sw, ph, pw, dh, dw;
  int wlayout;      // 0: [Cout][Cin][R*S] (PyTorch), 1: [R*S][Cout][Cin] (tap-major)
  int korder;       // forward / data-gradient K order: 0 tap-outer, 1 channel-chunk-outer
  int xcd;          // conv_lp.hip kernels: 1 = XCD-contiguous block order (xcd_block)
};

// XCD-contiguous logical block index: hardware block i runs on XCD i % 8 (a placement used for
// speed only, never for correctness); logical = the i-th block of that XCD's contiguous share
// of the grid, so neighbouring tiles (shared input rows, shared gradient rows) meet in one XCD's
// L2.  A bijection for any grid size.
__device__ __forceinline__ int xcd_linear(int i, int total) {
  const int q = total >> 3, r = total & 7, x = i & 7, j = i >> 3;
  return x * q + min(x, r) + j;
}

__device__ __forceinline__ void xcd_block(bool on, int &bx, int &by, int &bz) {
  bx = blockIdx.x;
  by = blockIdx.y;
  bz = blockIdx.z;
  if (!on) return;
  const int gx = gridDim.x, gy = gridDim.y;
  const int total = gx * gy * gridDim.z;
  const int L = xcd_linear(bx + gx * (by + gy * bz), total);
  bx = L % gx;
  by = (L / gx) % gy;
  bz = L / (gx * gy);
}

__host__ __device__ __forceinline__ int floordiv(int a, int b) {
  return a >= 0 ? a / b : -((-a + b - 1) / b);
}

// Tap liveness: does any output position o in [0, n_out) read an input o*step + d inside
// [0, n_in)?  A filter tap that never does only multiplies zero padding (the DeepLab ASPP
// branches at dilation 24 / 36 on 16x16 maps, reference model/convolutions.py:218-225: 8 of
// their 9 taps), so the GEMMs skip it: the sums are unchanged (those products are exact
// zeros) and the weight gradient of such a tap is exactly 0.
__host__ __device__ __forceinline__ bool axis_live(int d, int n_out, int step, int n_in) {
  if (n_out <= 0) return false;
  const int o0 = d >= 0 ? 0 : (-d + step - 1) / step;
  return o0 < n_out && o0 * step + d < n_in;
}

// live filter taps (axis_live on both axes): the weight-gradient GEMMs run over the columns
// (ci, live tap) only; the dead taps' gradient is written as 0 by the split reduction
struct TapList {
  int n;
  unsigned long long mask;  // bit tap = live (R*S <= MAXTAPS = 64)
  int tap[MAXTAPS];
};

// f(IntC<I>, IntC<J>) (common.h IntC), I / J = 2 where i2 / j2, else 1: the 2 x 2 tile choices
// of k_wgrad_1x1 (32- / 64-row wave tiles) and k_wgrad_lp (64- / 128-row tiles)
template <class F> inline void with_tile2x2(bool i2, bool j2, F f) {
  if (i2 && j2) f(IntC<2>(), IntC<2>());
  else if (i2) f(IntC<2>(), IntC<1>());
  else if (j2) f(IntC<1>(), IntC<2>());
  else f(IntC<1>(), IntC<1>());
}

// Launch plan of a weight gradient (conv.hip wgrad_plan: the one place that picks the kernel).
// Every kernel writes partial slabs part[split][Cout][Cin*R*S] for the fixed-order split
// reduction and accepts any splits >= 1 as a cap.
enum WgradKind { WGRAD_STEM, WGRAD_LP, WGRAD_1X1, WGRAD_GEN2, WGRAD_GEN1 };
struct WgradPlan {
  int kind;
  int op;      // operands: 1 bf16 (C3), 0 fp32 (conv.hip wgrad_op)
  int tm, tn;  // tile rows (Cout) x columns ((ci, live tap); k_wgrad_1x1: ci)
  int kstep;   // pixels per K-step (k_wgrad_1x1: its 8-pixel groups)
  int splits;  // default slab count (e2ep_conv_wgrad_splits)
  TapList tl;  // live taps
};
// a caller's splits -> per: pixels (k_wgrad_1x1: groups) per slab, used: slabs written
struct WgradGrid { int per, used; };

// Implicit-GEMM forward (mode 0) / data gradient (mode 1) with 32-deep K-steps and up to
// 128-row tiles, conv_lp.hip: bf16 / fp16 operands (op 1 / 2), and fp32 (op 0) where
// TUNE_LP32 selects it.  Tap-major weights ([R*S][Cout][Cin]) or 1x1 filters only.
struct LpPlan {
  int wm, wn, lk, splits, kper, nph;  // wave tiles (64 rows / columns each), K-step, K split
  long long ncols;                    // columns of the largest phase
};
bool lp_ok(int mode, const ConvGeom &g, int M, int op);
LpPlan lp_plan(int mode, const ConvGeom &g, int M, int op);
// lp_launch returns an E2EP status.  workspace: splits * M * ncols floats when p.splits > 1.
// stats (forward only): BatchNorm partial sums of dst from the epilogue (bnstats.h), over
// cdiv(ncols, 64 * wn) column tiles.
// io (e2ep.h E2EP_IO_*, op 1 only): mode 0 with E2EP_IO_X_BF16 reads a bf16 src, mode 1 with
// E2EP_IO_DX_BF16 writes a bf16 dst (dst_bytes: its size in bytes); E2EP_EINVAL otherwise.
int lp_launch(int mode, int act, int op, const float *w, const void *src, const float *bias,
              void *dst, long long dst_bytes, const ConvGeom &g, int M, const LpPlan &p,
              void *workspace, hipStream_t s, double *stats = nullptr, int io = 0);

// Weight gradient with 32-pixel K-steps and up to 128 x 128 tiles, conv_lp.hip: bf16 operands
// (op 1, C3) or fp32 (op 0, where TUNE_LP32W selects it).  lp_wgrad_plan fills p's tile, K-step
// and default splits from p.op and p.tl.
bool lp_wgrad_ok(const ConvGeom &g, const TapList &tl);
void lp_wgrad_plan(const ConvGeom &g, WgradPlan &p);
// xb: x is bf16 (op 1 only)
void lp_wgrad_launch(const float *gout, const void *x, const ConvGeom &g, const WgradPlan &p,
                     WgradGrid gr, float *part, hipStream_t s, bool xb = false);

// A conv layer's data gradient on k_conv_lp (plan p: CONV_LP / CONV_LP32 of conv.hip) and
// weight gradient (op 1: k_wgrad_lp; op 0: the k_conv_wgrad2-equivalent 64 x 64 tile) in one
// k_lp_bwd_pair launch (e2ep_conv_bwd).  lp_bwd_pair_ok says whether the two plans have an
// instantiated pair, and sets p's tile to the pair's.
bool lp_bwd_pair_ok(const ConvGeom &g, LpPlan &p, const WgradPlan &wp);
// xb: x and dx are bf16 (op 1 only; dx_bytes its size in bytes)
void lp_bwd_pair_launch(const float *w, const float *gout, const float *res, void *dx,
                        long long dx_bytes, const ConvGeom &g, int M, const LpPlan &p,
                        void *ws_dgrad, const void *x, const WgradPlan &wp, WgradGrid gr,
                        float *part2, hipStream_t s, bool xb = false);

// Direct convolution of a 7x7 / 2 conv with 64 output channels on 16-bit operands (op 1 / 2:
// the BEV stem in C3 / C5), conv_stem.hip: the forward (mode 0, k_conv_stem_lp) stages each
// output tile's input patch once per 16-channel chunk, the data gradient (mode 1, pad 3, 64
// gradient channels, k_conv_stem_dgrad_lp) each tile's gradient patch once.  Tap-major
// weights; e2ep_tune key 35 = 1 + mask (1 forward, 2 data gradient, 4 weight gradient; on fp32
// operands, op 0, also 8 for the gradients and 16 for the forward).  workspace: stem_direct_workspace(g, mode,
// op) bytes for the weight image (k_stem_wprep*).
bool stem_direct_ok(int mode, const ConvGeom &g, int M, int op);
size_t stem_direct_workspace(const ConvGeom &g, int mode, int op);
int stem_direct_launch(int act, int op, const float *w, const float *x, const float *bias, float *y,
                       long long y_bytes, const ConvGeom &g, void *workspace, hipStream_t s);
int stem_dgrad_launch(int op, const float *w, const float *gy, float *dx, long long dx_bytes,
                      const ConvGeom &g, void *workspace, hipStream_t s);
// mode 2: the weight gradient (k_conv_stem_wgrad_lp, op 1 bf16 / op 0 fp32 operands): split
// slabs part[split][64][Cin * 49] for the split reduction; returns the slabs written (-1: refused)
int stem_wgrad_splits(const ConvGeom &g);
int stem_wgrad_launch(const float *gy, const float *x, const ConvGeom &g, int splits, float *part,
                      hipStream_t s, int op);

}  // namespace e2ep
