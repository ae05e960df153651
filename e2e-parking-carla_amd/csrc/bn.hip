// BatchNorm2d (training: batch statistics; eval: running statistics) fused with the
// following activation, forward and backward, NCHW fp32, for gfx950.
//
// Replaces torch BatchNorm2d + ReLU / swish pairs throughout the hot path
// (efficientnet-pytorch MBConv _bn0/_bn1/_bn2 + swish, reference
// model/bev_encoder.py:14-20 bn1/relu and torchvision BasicBlock, model/convolutions.py
// ASPP/DeepLab/UpsamplingConcat conv-BN-ReLU, model/segmentation_head.py:26-31).
//
// Statistics are accumulated in fp64 (sum, sum of squares) from fixed per-workgroup slices
// and combined in a fixed order: biased variance for normalisation, unbiased for the
// running-variance update (PyTorch semantics), deterministic run to run.
// Backward recomputes the pre-activation from x (no saved activation tensor).
#include <algorithm>

#include "bns_layout.h"
#include "common.h"

// Contraction only within one expression (a*b + c -> fma): the fp32 and bf16-storage
// instantiations of a kernel (E2EP_IO_*) then fuse the same operations and round alike —
// under the default cross-statement contraction hipcc may pick a different multiply to fuse
// in each instantiation (tests/test_bf16_store_gpu.py holds them bitwise equal).
#pragma clang fp contract(on)

namespace e2ep {

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_SWISH = 2 };

__device__ __forceinline__ float act_fwd(float z, int act) {
  if (act == ACT_RELU) return fmaxf(z, 0.f);
  if (act == ACT_SWISH) return swish_f(z);
  return z;
}
// d act / dz
__device__ __forceinline__ float act_bwd(float z, int act) {
  if (act == ACT_RELU) return z > 0.f ? 1.f : 0.f;
  if (act == ACT_SWISH) {
    const float s = sigmoid_f(z);
    return s * (1.f + z * (1.f - s));
  }
  return 1.f;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Channel-major iteration: channel c's data is N rows of HW floats at stride C*HW.  Kernels
// walk it as one sequence of N*HWv vectors (VEC = 4 when HW % 4 == 0, else 1); vector t is
// row n = t / HWv, column p = t % HWv.
template <int VEC>
struct Vec;
template <>
struct Vec<4> {
  typedef float4 T;
  static __device__ __forceinline__ float4 ld(const float *p) { return *reinterpret_cast<const float4 *>(p); }
  static __device__ __forceinline__ float4 ld(const bf16_t *p) { return ld4(p); }
  static __device__ __forceinline__ void st(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
  static __device__ __forceinline__ void st(bf16_t *p, float4 v) { st4(p, v); }
  static __device__ __forceinline__ float get(const float4 &v, int i) {
    return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
  }
  static __device__ __forceinline__ void set(float4 &v, int i, float f) {
    if (i == 0) v.x = f; else if (i == 1) v.y = f; else if (i == 2) v.z = f; else v.w = f;
  }
  static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};
template <>
struct Vec<1> {
  typedef float T;
  static __device__ __forceinline__ float ld(const float *p) { return *p; }
  static __device__ __forceinline__ float ld(const bf16_t *p) { return ld1(p); }
  static __device__ __forceinline__ void st(float *p, float v) { *p = v; }
  static __device__ __forceinline__ void st(bf16_t *p, float v) { st1(p, v); }
  static __device__ __forceinline__ float get(const float &v, int) { return v; }
  static __device__ __forceinline__ void set(float &v, int, float f) { v = f; }
  static __device__ __forceinline__ float zero() { return 0.f; }
};

// (n, p) = divmod(t, HWv) for t = t0, t0 + 256, t0 + 512, ... (a 256-thread block's strided
// walk over a channel's N x HWv vectors): one division up front, then a carry per step instead
// of an integer division (~25 instructions) per vector
struct PlaneWalk {
  int n, p, dq, dr, hw;
  __device__ __forceinline__ PlaneWalk(int t0, int hw_) : hw(hw_) {
    n = t0 / hw;
    p = t0 - n * hw;
    dq = 256 / hw;
    dr = 256 - dq * hw;
  }
  __device__ __forceinline__ void next() {
    p += dr;
    n += dq;
    if (p >= hw) {
      p -= hw;
      ++n;
    }
  }
};

// fixed-order fp64 block reduction of two values (256 threads); result valid in every thread
__device__ __forceinline__ void block_sum2(double &s, double &q) {
  __shared__ double rs[4], rq[4];
  s = wave_sum_d(s);
  q = wave_sum_d(q);
  __syncthreads();  // rs/rq may still be read by a previous call
  if ((threadIdx.x & 63) == 0) {
    rs[threadIdx.x >> 6] = s;
    rq[threadIdx.x >> 6] = q;
  }
  __syncthreads();
  s = (rs[0] + rs[1]) + (rs[2] + rs[3]);
  q = (rq[0] + rq[1]) + (rq[2] + rq[3]);
}

// sum of channel c's `splits` partial pairs, fixed order (thread k takes entries k, k+256, ...)
__device__ __forceinline__ void channel_partials(const double *__restrict__ part, int c,
                                                 int splits, double &s, double &q) {
  s = 0.0;
  q = 0.0;
  for (int k = threadIdx.x; k < splits; k += 256) {
    s += part[((long long)c * splits + k) * 2 + 0];
    q += part[((long long)c * splits + k) * 2 + 1];
  }
  block_sum2(s, q);
}

// drop-connect (efficientnet-pytorch, training): out = bn / keep * floor(keep + u[n])
__device__ __forceinline__ float dc_scale(const float *dc_rand, float keep, int n, float z) {
  return dc_rand ? __fmul_rn(__fdiv_rn(z, keep), floorf(__fadd_rn(keep, dc_rand[n]))) : z;
}

// partial sums over a slice of channel c: grid (C, splits); slice = `per` vectors
template <int VEC, typename TX = float>
__global__ void __launch_bounds__(256) k_bn_stats(const TX *__restrict__ x, int N, int C,
                                                  int HWv, int splits, int per,
                                                  double *__restrict__ part) {
  const int c = blockIdx.x, sp = blockIdx.y;
  const int tot = N * HWv;
  const int beg = sp * per, end = min(tot, beg + per);
  double s = 0.0, q = 0.0;
  PlaneWalk w(beg + (int)threadIdx.x, HWv);
  for (int t = beg + threadIdx.x; t < end; t += 256, w.next()) {
    const int n = w.n, p = w.p;
    const auto v = Vec<VEC>::ld(x + (((size_t)n * C + c) * HWv + p) * VEC);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const double d = Vec<VEC>::get(v, i);
      s += d;
      q += d * d;
    }
  }
  block_sum2(s, q);
  if (threadIdx.x == 0) {
    part[((long long)c * splits + sp) * 2 + 0] = s;
    part[((long long)c * splits + sp) * 2 + 1] = q;
  }
}

// y = act(dc(gamma * (x - mean) * invstd + beta) + res); grid (C, chunks of `per` vectors).
// Train: mean / invstd from the stats partials (fp64, biased variance); chunk 0 of each
// channel publishes them and updates the running stats (unbiased variance).  Eval: from the
// running stats.
template <int VEC>
__global__ void __launch_bounds__(256) k_bn_apply(
    const float *__restrict__ x, const double *__restrict__ part, int splits, long long cnt,
    float eps, float momentum, float *__restrict__ running_mean, float *__restrict__ running_var,
    float *__restrict__ mean_out, float *__restrict__ invstd_out, const float *__restrict__ gamma,
    const float *__restrict__ beta, const float *__restrict__ res,
    const float *__restrict__ dc_rand, float dc_keep, int N, int C, int HWv, int per, int act,
    float *__restrict__ y, const float *__restrict__ scale, const float *__restrict__ shift,
    int rev) {
  // rev: back-to-front sweep, starting on the rows the producing conv wrote last (e2ep_tune 33)
  const int c = rev ? C - 1 - (int)blockIdx.x : (int)blockIdx.x;
  const int j = rev ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y;
  float mu = 0.f, is = 0.f;
  if (scale) {
    // folded affine from e2ep_bn_finalize_part / e2ep_bn_stats (bn_finalize_channel: the same
    // sc / sh expressions as below)
  } else if (part) {
    double s, q;
    channel_partials(part, c, splits, s, q);
    const double m = s / (double)cnt;
    double var = q / (double)cnt - m * m;
    if (var < 0.0) var = 0.0;
    mu = (float)m;
    is = (float)(1.0 / sqrt(var + (double)eps));
    if (j == 0 && threadIdx.x == 0) {
      mean_out[c] = mu;
      invstd_out[c] = is;
      if (running_mean) {
        const double unb = cnt > 1 ? var * (double)cnt / (double)(cnt - 1) : var;
        running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * m);
        running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unb);
      }
    }
  } else {
    mu = running_mean[c];
    is = (float)(1.0 / sqrt((double)running_var[c] + (double)eps));
    if (j == 0 && threadIdx.x == 0) {
      mean_out[c] = mu;
      invstd_out[c] = is;
    }
  }
  const float sc = scale ? scale[c] : is * (gamma ? gamma[c] : 1.f);
  const float sh = scale ? shift[c] : (beta ? beta[c] : 0.f) - mu * sc;
  const int tot = N * HWv;
  const int beg = j * per, end = min(tot, beg + per);
  PlaneWalk w(beg + (int)threadIdx.x, HWv);
  for (int t = beg + threadIdx.x; t < end; t += 256, w.next()) {
    const int n = w.n, p = w.p;
    const size_t off = (((size_t)n * C + c) * HWv + p) * VEC;
    auto v = Vec<VEC>::ld(x + off);
    const auto r = res ? Vec<VEC>::ld(res + off) : Vec<VEC>::zero();
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float z = dc_scale(dc_rand, dc_keep, n, Vec<VEC>::get(v, i) * sc + sh);
      Vec<VEC>::set(v, i, act_fwd(z + Vec<VEC>::get(r, i), act));
    }
    Vec<VEC>::st(y + off, v);
  }
}

// statistics only (for a consumer that applies the normalisation on load, e.g. the depthwise
// conv): mean / invstd, the folded scale / shift (sc = gamma * invstd, sh = beta - mean * sc,
// the same arithmetic as k_bn_apply) and the running-stat update of channel c; every thread
// of the block calls it (block-wide partial sum), thread 0 writes
__device__ __forceinline__ void bn_finalize_channel(
    int c, const double *__restrict__ part, int splits, long long cnt, float eps, float momentum,
    float *__restrict__ running_mean, float *__restrict__ running_var, float *__restrict__ mean_out,
    float *__restrict__ invstd_out, const float *__restrict__ gamma, const float *__restrict__ beta,
    float *__restrict__ scale, float *__restrict__ shift) {
  float mu, is;
  if (part) {
    double s, q;
    channel_partials(part, c, splits, s, q);
    if (threadIdx.x != 0) return;
    const double m = s / (double)cnt;
    double var = q / (double)cnt - m * m;
    if (var < 0.0) var = 0.0;
    mu = (float)m;
    is = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
      const double unb = cnt > 1 ? var * (double)cnt / (double)(cnt - 1) : var;
      running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * m);
      running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unb);
    }
  } else {
    if (threadIdx.x != 0) return;
    mu = running_mean[c];
    is = (float)(1.0 / sqrt((double)running_var[c] + (double)eps));
  }
  mean_out[c] = mu;
  invstd_out[c] = is;
  const float sc = is * (gamma ? gamma[c] : 1.f);
  scale[c] = sc;
  shift[c] = (beta ? beta[c] : 0.f) - mu * sc;
}

// Finalize from a producer's tile-major partials (bnstats.h: part[(tile * C + c) * 2]):
// block = 8 channels x 128 tile groups (lane = tid % 8 -> channel c0 + lane, group = tid / 8):
// the 8 lanes of a group read one 128-B line per tile (channels c0 .. c0+7), group j sums tiles
// j, j + 128, ...; the group sums are added in group order through LDS, then the statistics
// as bn_finalize_channel computes them.  grid = C / 8.  Fixed order: deterministic.  (A
// two-level version that spread each channel's tiles over workgroups and handed the range
// sums to the last-arriving one spent 12.7 us per launch on the hand-off's uncached loads.)
constexpr int FT_CH = 8, FT_GROUPS = 128;  // 1024 threads: a few loads per thread, all in flight
__global__ void __launch_bounds__(FT_CH * FT_GROUPS) k_bn_finalize_tiles(
    const double *__restrict__ part, int tiles, int C, long long cnt, float eps, float momentum,
    float *__restrict__ running_mean, float *__restrict__ running_var,
    float *__restrict__ mean_out, float *__restrict__ invstd_out, const float *__restrict__ gamma,
    const float *__restrict__ beta, float *__restrict__ scale, float *__restrict__ shift) {
  __shared__ double rs[FT_GROUPS][FT_CH], rq[FT_GROUPS][FT_CH];
  const int lane = threadIdx.x % FT_CH, grp = threadIdx.x / FT_CH;
  const int c = blockIdx.x * FT_CH + lane;
  double s = 0.0, q = 0.0;
  if (c < C) {
#pragma unroll 4
    for (int k = grp; k < tiles; k += FT_GROUPS) {
      const double2 v = *reinterpret_cast<const double2 *>(part + ((size_t)k * C + c) * 2);
      s += v.x;
      q += v.y;
    }
  }
  rs[grp][lane] = s;
  rq[grp][lane] = q;
  __syncthreads();
  // fixed two-level order: groups j, j + 16, ..., j + 112 for j < 16, then the 16 in order
  double s2 = 0.0, q2 = 0.0;
  if (grp < 16) {
    s2 = rs[grp][lane];
    q2 = rq[grp][lane];
    for (int j = grp + 16; j < FT_GROUPS; j += 16) {
      s2 += rs[j][lane];
      q2 += rq[j][lane];
    }
  }
  __syncthreads();  // every thread: the first-level sums are read before they are overwritten
  if (grp < 16) {
    rs[grp][lane] = s2;
    rq[grp][lane] = q2;
  }
  __syncthreads();
  if (grp != 0 || c >= C) return;
  double S = rs[0][lane], Q = rq[0][lane];
  for (int j = 1; j < 16; ++j) {
    S += rs[j][lane];
    Q += rq[j][lane];
  }
  const double m = S / (double)cnt;
  double var = Q / (double)cnt - m * m;
  if (var < 0.0) var = 0.0;
  const float mu = (float)m;
  const float is = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const double unb = cnt > 1 ? var * (double)cnt / (double)(cnt - 1) : var;
    running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * m);
    running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unb);
  }
  mean_out[c] = mu;
  invstd_out[c] = is;
  const float sc = is * (gamma ? gamma[c] : 1.f);
  scale[c] = sc;
  shift[c] = (beta ? beta[c] : 0.f) - mu * sc;
}

// Eval statistics of many BatchNorm layers in one launch (e2ep_bn_eval_multi): block = one
// table row {running_mean, running_var, gamma, beta, out, C, eps bits}; out = [mean | invstd |
// scale | shift] (4 x C), the arithmetic of bn_finalize_channel's eval branch.
__global__ void __launch_bounds__(256) k_bn_eval_multi(const long long *__restrict__ tab) {
  const long long *r = tab + 7LL * blockIdx.x;
  const float *rm = reinterpret_cast<const float *>(r[0]);
  const float *rv = reinterpret_cast<const float *>(r[1]);
  const float *gamma = reinterpret_cast<const float *>(r[2]);
  const float *beta = reinterpret_cast<const float *>(r[3]);
  float *out = reinterpret_cast<float *>(r[4]);
  const int C = (int)r[5];
  const float eps = __builtin_bit_cast(float, (int)r[6]);
  for (int c = threadIdx.x; c < C; c += 256) {
    const float mu = rm[c];
    const float is = (float)(1.0 / sqrt((double)rv[c] + (double)eps));
    const float sc = is * (gamma ? gamma[c] : 1.f);
    out[c] = mu;
    out[C + c] = is;
    out[2 * C + c] = sc;
    out[3 * C + c] = (beta ? beta[c] : 0.f) - mu * sc;
  }
}

// grid (C): eval (part == null) or a separate finalize after k_bn_stats
__global__ void __launch_bounds__(256) k_bn_finalize(
    const double *__restrict__ part, int splits, long long cnt, float eps, float momentum,
    float *__restrict__ running_mean, float *__restrict__ running_var, float *__restrict__ mean_out,
    float *__restrict__ invstd_out, const float *__restrict__ gamma, const float *__restrict__ beta,
    float *__restrict__ scale, float *__restrict__ shift) {
  bn_finalize_channel(blockIdx.x, part, splits, cnt, eps, momentum, running_mean, running_var,
                      mean_out, invstd_out, gamma, beta, scale, shift);
}

// squeeze-excitation gate downstream of the activation (e2ep_bn_bwd gate_logit /
// gate_dpooled): the gradient at the activation output is dy * sigmoid(logit[n,c]) +
// dpooled[n,c] / HW (the SE op's dx, se.hip k_se_dx, formed here instead of stored)
struct BnGate {
  const float *logit, *dpooled;
  float inv_hw;
  __device__ __forceinline__ bool on() const { return logit != nullptr; }
  __device__ __forceinline__ void coef(int n, int C, int c, float &s, float &d) const {
    const int i = n * C + c;
    s = sigmoid_f(logit[i]);
    d = dpooled[i] * inv_hw;
  }
};
template <int VEC>
__device__ __forceinline__ typename Vec<VEC>::T gate_dy(typename Vec<VEC>::T dv, const BnGate &gt,
                                                        int n, int C, int c) {
  if (gt.on()) {
    float s, d;
    gt.coef(n, C, c, s, d);
#pragma unroll
    for (int i = 0; i < VEC; ++i) Vec<VEC>::set(dv, i, Vec<VEC>::get(dv, i) * s + d);
  }
  return dv;
}

// backward pieces shared by reduce and apply: from x, dy (and res / drop-connect), returns
// xhat, dz (gradient at the activation input = dres) and dzb (gradient at the BN output)
template <int VEC>
struct BnBwdElem {
  float mu, is, g, b;
  const float *dc_rand;
  float keep;
  int act;
  __device__ __forceinline__ void operator()(float xv, float dyv, float rv, int n, float &xh,
                                             float &dz, float &dzb) const {
    xh = (xv - mu) * is;
    const float zb = xh * g + b;
    dz = dyv * act_bwd(dc_scale(dc_rand, keep, n, zb) + rv, act);
    dzb = dc_rand ? __fdiv_rn(__fmul_rn(dz, floorf(__fadd_rn(keep, dc_rand[n]))), keep) : dz;
  }
  // the same with the sample's drop-connect factor floor(keep + u[n]) loaded beforehand
  __device__ __forceinline__ void with_factor(float xv, float dyv, float rv, float dcf, float &xh,
                                              float &dz, float &dzb) const {
    xh = (xv - mu) * is;
    const float zb = xh * g + b;
    const float zs = dc_rand ? __fmul_rn(__fdiv_rn(zb, keep), dcf) : zb;
    dz = dyv * act_bwd(zs + rv, act);
    dzb = dc_rand ? __fdiv_rn(__fmul_rn(dz, dcf), keep) : dz;
  }
};

// per-vector sample factors of the single-launch kernels, loaded before the channel data:
// a per-element `dc_rand[n]` / gate read inside the element loop made hipcc wait vmcnt(0)
// (the counters are in order) behind every x / dy load, one round trip per vector (the
// single-launch backward ran at 1.7 TB/s, round 3)
template <int T, int R>
__device__ __forceinline__ void bns_factors(int tot, int HWv, int C, int c, const float *dc_rand,
                                            float keep, const BnGate *gt, float (&dcf)[R],
                                            float (&gs)[R], float (&gd)[R]) {
  int n[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    n[u] = min((int)threadIdx.x + u * T, tot - 1) / HWv;
    dcf[u] = 1.f;
    gs[u] = 1.f;
    gd[u] = 0.f;
  }
  // raw loads only (uniform branches); bns_factors_finish does the arithmetic once the
  // caller has issued its channel loads too, so every load of the block is in flight at once
  if (dc_rand) {
#pragma unroll
    for (int u = 0; u < R; ++u) dcf[u] = dc_rand[n[u]];
  }
  if (gt && gt->on()) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      gs[u] = gt->logit[n[u] * C + c];
      gd[u] = gt->dpooled[n[u] * C + c];
    }
  }
}
template <int R>
__device__ __forceinline__ void bns_factors_finish(const float *dc_rand, float keep,
                                                   const BnGate *gt, float (&dcf)[R],
                                                   float (&gs)[R], float (&gd)[R]) {
  if (dc_rand) {
#pragma unroll
    for (int u = 0; u < R; ++u) dcf[u] = floorf(__fadd_rn(keep, dcf[u]));
  }
  if (gt && gt->on()) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      gs[u] = sigmoid_f(gs[u]);  // = BnGate::coef
      gd[u] = gd[u] * gt->inv_hw;
    }
  }
}

// backward reduction: per channel sums of dzb and dzb * xhat (fp64); grid (C, splits)
template <int VEC, typename TX = float, typename TD = float>
__global__ void __launch_bounds__(256) k_bn_bwd_reduce(
    const TX *__restrict__ x, const TD *__restrict__ dy, const float *__restrict__ mean,
    const float *__restrict__ invstd, const float *__restrict__ gamma,
    const float *__restrict__ beta, const float *__restrict__ res,
    const float *__restrict__ dc_rand, float dc_keep, BnGate gt, int N, int C, int HWv,
    int splits, int per, int act, double *__restrict__ part, int rev) {
  // rev: walk the tensor back to front (blocks are dispatched x fastest, so the forward order
  // sweeps memory front to back; e2ep_tune key 33)
  const int c = rev ? C - 1 - (int)blockIdx.x : (int)blockIdx.x;
  const int sp = rev ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y;
  const int tot = N * HWv;
  const int beg = sp * per, end = min(tot, beg + per);
  const BnBwdElem<VEC> el{mean[c], invstd[c], gamma ? gamma[c] : 1.f, beta ? beta[c] : 0.f,
                          dc_rand, dc_keep, act};
  double s = 0.0, q = 0.0;
  PlaneWalk w(beg + (int)threadIdx.x, HWv);
  for (int t = beg + threadIdx.x; t < end; t += 256, w.next()) {
    const int n = w.n, p = w.p;
    const size_t off = (((size_t)n * C + c) * HWv + p) * VEC;
    const auto xv = Vec<VEC>::ld(x + off);
    const auto dv = gate_dy<VEC>(Vec<VEC>::ld(dy + off), gt, n, C, c);
    const auto rv = res ? Vec<VEC>::ld(res + off) : Vec<VEC>::zero();
    // a vector's VEC terms summed in fp32 first, then into the fp64 sums (one fp64 add per
    // vector and sum instead of an add, a multiply and two conversions per element)
    float s4 = 0.f, q4 = 0.f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      float xh, dz, dzb;
      el(Vec<VEC>::get(xv, i), Vec<VEC>::get(dv, i), Vec<VEC>::get(rv, i), n, xh, dz, dzb);
      s4 += dzb;
      q4 = __builtin_fmaf(dzb, xh, q4);
    }
    s += s4;
    q += q4;
  }
  block_sum2(s, q);
  if (threadIdx.x == 0) {
    part[((long long)c * splits + sp) * 2 + 0] = s;
    part[((long long)c * splits + sp) * 2 + 1] = q;
  }
}

// dbeta[c] = sum dzb, dgamma[c] = sum dzb*xhat: only when no dx / dres is wanted
__global__ void __launch_bounds__(256) k_bn_bwd_finalize(const double *__restrict__ part,
                                                         int splits, float *__restrict__ dgamma,
                                                         float *__restrict__ dbeta) {
  const int c = blockIdx.x;
  double s, q;
  channel_partials(part, c, splits, s, q);
  if (threadIdx.x == 0) {
    if (dbeta) dbeta[c] = (float)s;
    if (dgamma) dgamma[c] = (float)q;
  }
}

// dres = dz;  dx = gamma * invstd * (dzb - (sum_dzb + xhat * sum_dzbxhat) / M)   (train)
//             dx = gamma * invstd * dzb                                          (eval)
// grid (C, chunks); chunk 0 of each channel writes dgamma / dbeta.
template <int VEC, typename TX = float, typename TD = float, typename TO = float>
__global__ void __launch_bounds__(256) k_bn_bwd_apply(
    const TX *__restrict__ x, const TD *__restrict__ dy, const float *__restrict__ mean,
    const float *__restrict__ invstd, const float *__restrict__ gamma,
    const float *__restrict__ beta, const float *__restrict__ res,
    const float *__restrict__ dc_rand, float dc_keep, BnGate gt, const double *__restrict__ part,
    int splits, long long cnt, int N, int C, int HWv, int per, int act, int train,
    TO *__restrict__ dx, float *__restrict__ dres, float *__restrict__ dgamma,
    float *__restrict__ dbeta, const double *__restrict__ planes, int rev) {
  // rev: back-to-front sweep, so the apply pass starts on the rows the reduction (or the
  // producer) touched last, while they may still sit in the 256 MB MALL (e2ep_tune key 33)
  const int c = rev ? C - 1 - (int)blockIdx.x : (int)blockIdx.x;
  const int j = rev ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y;
  double s, q;
  if (planes) {  // e2ep_bn_bwd_planes: the sums from the SE pass's per-plane factors
    s = 0.0;
    q = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
      float gs, gd;
      gt.coef(n, C, c, gs, gd);
      const double *a = planes + 4LL * ((long long)n * C + c);
      s += (double)gs * a[0] + (double)gd * a[1];
      q += (double)gs * a[2] + (double)gd * a[3];
    }
    block_sum2(s, q);
  } else {
    channel_partials(part, c, splits, s, q);
  }
  if (j == 0 && threadIdx.x == 0) {
    if (dbeta) dbeta[c] = (float)s;
    if (dgamma) dgamma[c] = (float)q;
  }
  const float ms = (float)(s / (double)cnt), mq = (float)(q / (double)cnt);
  const BnBwdElem<VEC> el{mean[c], invstd[c], gamma ? gamma[c] : 1.f, beta ? beta[c] : 0.f,
                          dc_rand, dc_keep, act};
  const float gis = el.g * el.is;
  const int tot = N * HWv;
  const int beg = j * per, end = min(tot, beg + per);
  PlaneWalk w(beg + (int)threadIdx.x, HWv);
  for (int t = beg + threadIdx.x; t < end; t += 256, w.next()) {
    const int n = w.n, p = w.p;
    const size_t off = (((size_t)n * C + c) * HWv + p) * VEC;
    const auto xv = Vec<VEC>::ld(x + off);
    const auto dv = gate_dy<VEC>(Vec<VEC>::ld(dy + off), gt, n, C, c);
    const auto rv = res ? Vec<VEC>::ld(res + off) : Vec<VEC>::zero();
    auto ox = Vec<VEC>::zero(), orr = Vec<VEC>::zero();
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      float xh, dz, dzb;
      el(Vec<VEC>::get(xv, i), Vec<VEC>::get(dv, i), Vec<VEC>::get(rv, i), n, xh, dz, dzb);
      Vec<VEC>::set(orr, i, dz);
      Vec<VEC>::set(ox, i, gis * (train ? dzb - (ms + xh * mq) : dzb));
    }
    if (dres) Vec<VEC>::st(dres + off, orr);
    if (dx) Vec<VEC>::st(dx + off, ox);
  }
}

// ------------------------------------------------------------------------------------------
// Single-launch BatchNorm for channels of at most BNS_T * 4 * BNS_R = 8192 elements (N * H * W:
// the 16x16 EfficientNet stages and the BEV encoder's deepest layers): one 256-thread block per
// channel holds the channel in registers from
// the statistics to the normalisation, so forward is one launch and one read of x (instead of
// stats + apply / finalize), backward one launch and one read of x, dy (instead of reduce +
// apply).  Same fp64 statistics and element arithmetic as the split kernels above; the
// summation is in a fixed order (thread t takes vectors t, t + 1024, ...), so deterministic.
// ------------------------------------------------------------------------------------------
// (BNS_T, BNS_R and the <threads, vectors per thread> layouts: bns_layout.h)

template <int T>
__device__ __forceinline__ void block_sum2_t(double &s, double &q) {
  constexpr int NW = T / 64;
  __shared__ double rs[NW], rq[NW];
  s = wave_sum_d(s);
  q = wave_sum_d(q);
  if ((threadIdx.x & 63) == 0) {
    rs[threadIdx.x >> 6] = s;
    rq[threadIdx.x >> 6] = q;
  }
  __syncthreads();
  s = 0.0;
  q = 0.0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    s += rs[i];
    q += rq[i];
  }
}

// float offset of float4 vector t of channel c (row n = t / HWv)
__device__ __forceinline__ size_t bns_off(int t, int HWv, int C, int c) {
  const int n = t / HWv, p = t - n * HWv;
  return (((size_t)n * C + c) * HWv + p) * 4;
}

// train-mode forward; y == null: statistics only (scale / shift for an apply-on-load consumer)
template <int T, int R, typename TX = float>
__global__ void __launch_bounds__(T) k_bn_fwd_small(
    const TX *__restrict__ x, long long cnt, float eps, float momentum,
    float *__restrict__ running_mean, float *__restrict__ running_var, float *__restrict__ mean_out,
    float *__restrict__ invstd_out, const float *__restrict__ gamma, const float *__restrict__ beta,
    const float *__restrict__ res, const float *__restrict__ dc_rand, float dc_keep, int N, int C,
    int HWv, int act, float *__restrict__ y, float *__restrict__ scale, float *__restrict__ shift) {
  const int c = blockIdx.x, tot = N * HWv;
  float dcf[R], gs[R], gd[R];
  if (y) bns_factors<T, R>(tot, HWv, C, c, dc_rand, dc_keep, nullptr, dcf, gs, gd);
  float4 v[R];
#pragma unroll
  for (int u = 0; u < R; ++u) v[u] = Vec<4>::ld(x + bns_off(min((int)threadIdx.x + u * T, tot - 1), HWv, C, c));
  double s = 0.0, q = 0.0;
#pragma unroll
  for (int u = 0; u < R; ++u) {
    if ((int)threadIdx.x + u * T >= tot) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double d = Vec<4>::get(v[u], i);
      s += d;
      q += d * d;
    }
  }
  block_sum2_t<T>(s, q);
  const double m = s / (double)cnt;
  double var = q / (double)cnt - m * m;
  if (var < 0.0) var = 0.0;
  const float mu = (float)m, is = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = is * (gamma ? gamma[c] : 1.f);
  const float sh = (beta ? beta[c] : 0.f) - mu * sc;
  if (threadIdx.x == 0) {
    mean_out[c] = mu;
    invstd_out[c] = is;
    if (scale) {
      scale[c] = sc;
      shift[c] = sh;
    }
    if (running_mean) {
      const double unb = cnt > 1 ? var * (double)cnt / (double)(cnt - 1) : var;
      running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * m);
      running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unb);
    }
  }
  if (!y) return;
  float4 rr[R];
#pragma unroll
  for (int u = 0; u < R; ++u)
    rr[u] = res ? Vec<4>::ld(res + bns_off(min((int)threadIdx.x + u * T, tot - 1), HWv, C, c))
                : Vec<4>::zero();
  bns_factors_finish<R>(dc_rand, dc_keep, nullptr, dcf, gs, gd);
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int t = threadIdx.x + u * T;
    if (t >= tot) break;
    const size_t off = bns_off(t, HWv, C, c);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float zb = Vec<4>::get(v[u], i) * sc + sh;
      const float z = dc_rand ? __fmul_rn(__fdiv_rn(zb, dc_keep), dcf[u]) : zb;  // = dc_scale
      Vec<4>::set(v[u], i, act_fwd(z + Vec<4>::get(rr[u], i), act));
    }
    Vec<4>::st(y + off, v[u]);
  }
}

template <int T, int R, typename TX = float, typename TD = float, typename TO = float>
__global__ void __launch_bounds__(T) k_bn_bwd_small(
    const TX *__restrict__ x, const TD *__restrict__ dy, const float *__restrict__ mean,
    const float *__restrict__ invstd, const float *__restrict__ gamma,
    const float *__restrict__ beta, const float *__restrict__ res,
    const float *__restrict__ dc_rand, float dc_keep, BnGate gt, long long cnt, int N, int C,
    int HWv, int act, int train, TO *__restrict__ dx, float *__restrict__ dres,
    float *__restrict__ dgamma, float *__restrict__ dbeta) {
  const int c = blockIdx.x, tot = N * HWv;
  const BnBwdElem<4> el{mean[c], invstd[c], gamma ? gamma[c] : 1.f, beta ? beta[c] : 0.f,
                        dc_rand, dc_keep, act};
  float dcf[R], gs[R], gd[R];
  bns_factors<T, R>(tot, HWv, C, c, dc_rand, dc_keep, &gt, dcf, gs, gd);
  float4 xv[R], dv[R], rv[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const size_t off = bns_off(min((int)threadIdx.x + u * T, tot - 1), HWv, C, c);
    xv[u] = Vec<4>::ld(x + off);
    dv[u] = Vec<4>::ld(dy + off);
    rv[u] = res ? Vec<4>::ld(res + off) : Vec<4>::zero();
  }
  bns_factors_finish<R>(dc_rand, dc_keep, &gt, dcf, gs, gd);
  // one pass of the element math (act derivative: an exp and a divide for swish) whose results
  // stay in registers for the apply below (the block holds one channel: registers are free)
  float xh[R][4], dz[R][4], dzb[R][4];
  double s = 0.0, q = 0.0;
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int t = threadIdx.x + u * T;
    float s4 = 0.f, q4 = 0.f;  // fp32 over the vector, then fp64 (as k_bn_bwd_reduce)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      el.with_factor(Vec<4>::get(xv[u], i), Vec<4>::get(dv[u], i) * gs[u] + gd[u],
                     Vec<4>::get(rv[u], i), dcf[u], xh[u][i], dz[u][i], dzb[u][i]);
      s4 += dzb[u][i];
      q4 = __builtin_fmaf(dzb[u][i], xh[u][i], q4);
    }
    if (t < tot) {
      s += s4;
      q += q4;
    }
  }
  block_sum2_t<T>(s, q);
  if (threadIdx.x == 0) {
    if (dbeta) dbeta[c] = (float)s;
    if (dgamma) dgamma[c] = (float)q;
  }
  if (!dx && !dres) return;
  const float ms = (float)(s / (double)cnt), mq = (float)(q / (double)cnt);
  const float gis = el.g * el.is;
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int t = threadIdx.x + u * T;
    if (t >= tot) break;
    const size_t off = bns_off(t, HWv, C, c);
    float4 ox, orr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      Vec<4>::set(orr, i, dz[u][i]);
      Vec<4>::set(ox, i, gis * (train ? dzb[u][i] - (ms + xh[u][i] * mq) : dzb[u][i]));
    }
    if (dres) Vec<4>::st(dres + off, orr);
    if (dx) Vec<4>::st(dx + off, ox);
  }
}

// elementwise activation forward/backward (for activations not fused into a BN)
__global__ void k_act_fwd(const float *__restrict__ x, long long n, int act, float *__restrict__ y) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = act_fwd(x[i], act);
}
__global__ void k_act_bwd(const float *__restrict__ x, const float *__restrict__ dy, long long n,
                          int act, float *__restrict__ dx) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dx[i] = dy[i] * act_bwd(x[i], act);
}

// ------------------------------------------------------------------------------------------
// Host half.  bn_plan() is the only place that says which kernels run for a shape, on which
// layout and grid; the queries and the launch entry points read what it returns.
// ------------------------------------------------------------------------------------------
static int g_bn_small = 1;  // e2ep_bn_small(0) routes every shape to the split kernels (tests, A/B)
// largest channel (in float4 vectors) the single-launch kernels take, forward / backward
// (e2ep_bn_small_limits, A/B timing; at most BNS_R * BNS_T).  In the replayed C2 step, blocks
// of 1024 threads for channels up to 32768 elements measured 0.25 ms/step slower than the
// split kernels there (25.45 vs 25.19 ms, profiles/r02/session6/wgrad_target_bn_limits_ab.txt),
// so only the 256-thread shapes take the single launch.
static int g_bns_fwd_max = BNS_R * BNS_T, g_bns_bwd_max = BNS_R * BNS_T;

struct BnGeom {
  bool valid;       // N, C, H, W > 0; nothing below is set otherwise
  int N, C, HW;
  bool v4;          // float4 accesses: H * W % 4 == 0 (and `aligned`)
  int HWv, totv;    // vectors (v4) or elements of a plane / of a channel
  long long per_c;  // elements of a channel
};
// aligned: e2ep_bn_apply alone folds the 16-byte alignment of x, y and res into v4; every other
// entry point takes H * W % 4 == 0 as enough
static BnGeom bn_geom(int N, int C, int H, int W, bool aligned = true) {
  BnGeom g{};
  g.valid = N > 0 && C > 0 && H > 0 && W > 0;
  if (!g.valid) return g;
  g.N = N, g.C = C, g.HW = H * W;
  g.per_c = (long long)N * H * W;
  g.v4 = (g.HW & 3) == 0 && aligned;
  g.HWv = g.v4 ? g.HW / 4 : g.HW;
  g.totv = (int)((long long)N * g.HWv);
  return g;
}

struct BnPlan {
  BnGeom g;
  // Single launch (k_bn_fwd_small / k_bn_bwd_small) and its layout; {0, 0}: the split route.
  // e2ep_bn_fwd / e2ep_bn_stats take `fwd` only when train: eval goes straight to apply /
  // finalize with part = nullptr, sp = 1.  e2ep_bn_bwd_planes never takes `bwd`.
  BnsLayout fwd, bwd;
  // Split route.  The workspace is sized from the requested `splits`, not from the smaller
  // effective sp.  Forward and statistics demand it whenever train, even where `fwd` is
  // taken; the backward only where `bwd` is not.
  int splits;        // e2ep_tune key 0 workgroups over the C channels, each of >= key-1 elements; 1 .. 256
  size_t workspace;  // C x splits x 2 doubles
  bool launch_ok;    // what a launch needs besides g.valid: C <= 65535, N * H * W < 2^31; the
                     // fields below are set only then (and fwd / bwd are {0, 0} otherwise)
  int sp, per;       // slices per channel of `per` vectors: grid (C, sp) of k_bn_stats / k_bn_bwd_reduce
  int apply_per, apply_blocks;  // vectors per apply workgroup (4 per thread; e2ep_tune key 2): grid (C, apply_blocks)
  // sweep direction of the split passes (e2ep_tune key 33 = 1 + mask): mask bit 0 backward
  // apply back to front, bit 1 backward reduction back to front, bit 2 forward apply back to front
  int rev_apply, rev_reduce, rev_fwd;
};

static BnPlan bn_plan(const BnGeom &g) {
  BnPlan p{};
  p.g = g;
  if (!g.valid) return p;
  const long long want = (g_tune[TUNE_BN_SPLIT_TARGET] + g.C - 1) / g.C;
  const long long cap = g.per_c / g_tune[TUNE_BN_SPLIT_MIN];
  p.splits = (int)std::max(1LL, std::min({want, cap, 256LL}));
  p.workspace = (size_t)g.C * p.splits * 2 * sizeof(double);
  p.launch_ok = g.C <= 65535 && g.per_c < (1LL << 31);
  if (!p.launch_ok) return p;
  if (g.v4 && g_bn_small != 0) {
    if (g.totv <= g_bns_fwd_max) p.fwd = bns_layout(g.totv);
    if (g.totv <= g_bns_bwd_max) p.bwd = bns_layout(g.totv);
  }
  p.per = cdiv(g.totv, p.splits);
  p.sp = cdiv(g.totv, p.per);
  p.apply_per = g_tune[TUNE_BN_APPLY_PER];
  p.apply_blocks = cdiv(g.totv, p.apply_per);
  const int order = g_tune[TUNE_BN_ORDER] - 1;
  p.rev_apply = order & 1, p.rev_reduce = (order >> 1) & 1, p.rev_fwd = (order >> 2) & 1;
  return p;
}

// What every launch entry point requires of its shape and, where need_ws, of its workspace
// (0, or the status to hand back)
static int bn_check(const char *fn, const BnPlan &p, bool need_ws = false,
                    const void *workspace = nullptr, size_t workspace_bytes = 0) {
  E2EP_REQUIRE(p.launch_ok, E2EP_EINVAL, "%s: bad shape", fn);
  E2EP_REQUIRE(!need_ws || (workspace && workspace_bytes >= p.workspace), E2EP_EINVAL,
               "%s: workspace %zu bytes < %zu (e2ep_bn_workspace)", fn, workspace_bytes, p.workspace);
  return 0;
}

// storage types of (x, dy, dx) for an io mask (e2ep.h E2EP_IO_*): fp32, or the bf16
// combinations the step stores — the depthwise output's BN (_bn1: x and dx bf16, dy bf16 too
// when the squeeze-excitation output is stored bf16) and the expand output's BN (_bn0: the
// depthwise data gradient dy bf16)
enum BnIo {
  BNIO_F32 = 0,
  BNIO_XDX = E2EP_IO_X_BF16 | E2EP_IO_DX_BF16,
  BNIO_ALL = E2EP_IO_X_BF16 | E2EP_IO_DY_BF16 | E2EP_IO_DX_BF16,
  BNIO_DY = E2EP_IO_DY_BF16
};
static bool bn_io_ok(int io) {
  return io == BNIO_F32 || io == BNIO_XDX || io == BNIO_ALL || io == BNIO_DY;
}

// ---- template dispatch: f is a generic lambda (integral constants: common.h IntC) -----------
// f(VEC), VEC = 4 or 1
template <class F> static void with_vec(bool v4, F f) {
  if (v4) f(IntC<4>());
  else f(IntC<1>());
}
// f(T, R) for the seven layouts bns_layout() gives
template <class F> static void with_layout(BnsLayout l, F f) {
  IntC<BNS_T> t1;
  IntC<2 * BNS_T> t2;
  if (l.T == BNS_T && l.R == 1) f(t1, IntC<1>());
  else if (l.T == BNS_T && l.R == 2) f(t1, IntC<2>());
  else if (l.T == BNS_T && l.R == 4) f(t1, IntC<4>());
  else if (l.T == BNS_T) f(t1, IntC<8>());
  else if (l.R == 1) f(t2, IntC<1>());
  else if (l.R == 2) f(t2, IntC<2>());
  else f(t2, IntC<4>());
}
// f(x, dy, dx) as typed pointers for the four storage combinations of BnIo
template <class F> static void with_bn_io(int io, const void *x, const void *dy, void *dx, F f) {
  const float *xf = static_cast<const float *>(x), *dyf = static_cast<const float *>(dy);
  const bf16_t *xb = static_cast<const bf16_t *>(x), *dyb = static_cast<const bf16_t *>(dy);
  if (io == BNIO_XDX) f(xb, dyf, static_cast<bf16_t *>(dx));
  else if (io == BNIO_ALL) f(xb, dyb, static_cast<bf16_t *>(dx));
  else if (io == BNIO_DY) f(xf, dyb, static_cast<float *>(dx));
  else f(xf, dyf, static_cast<float *>(dx));
}
template <class P> using elem_t = std::remove_const_t<std::remove_pointer_t<P>>;
// The entry points refuse bf16 storage unless H * W % 4 == 0, so no VEC = 1 kernel with a bf16
// storage type is built
template <int VEC, class... Ts>
constexpr bool bn_built = VEC == 4 || (std::is_same<Ts, float>::value && ...);

// what the forward kernels share: the statistics' arguments, the elementwise tail
// y = act(dc(z) + res) (e2ep_bn_stats has none: y null) and the folded affine it writes instead
struct BnFwd {
  float eps, momentum;
  float *running_mean, *running_var, *mean, *invstd;
  const float *gamma, *beta, *res, *dc_rand;
  float dc_keep;
  int act;
  float *y, *scale, *shift;
};

// e2ep_bn_fwd and e2ep_bn_stats.  Training: the single launch where the plan takes it, else
// k_bn_stats into the workspace and the caller's tail (k_bn_apply / k_bn_finalize) on those
// partial sums.  Eval goes straight to the tail with no partial sums.
template <typename TX, class Tail>
static int bn_fwd_run(const char *fn, const BnPlan &p, const TX *x, int train, const BnFwd &a,
                      void *workspace, hipStream_t s, Tail tail) {
  const BnGeom &g = p.g;
  if (train && p.fwd.T) {
    with_layout(p.fwd, [&](auto t, auto r) {
      constexpr int T = decltype(t)::value;
      hipLaunchKernelGGL((k_bn_fwd_small<T, decltype(r)::value, TX>), dim3(g.C), dim3(T), 0, s, x,
                         g.per_c, a.eps, a.momentum, a.running_mean, a.running_var, a.mean, a.invstd,
                         a.gamma, a.beta, a.res, a.dc_rand, a.dc_keep, g.N, g.C, g.HWv, a.act, a.y,
                         a.scale, a.shift);
    });
  } else if (train) {
    double *part = static_cast<double *>(workspace);
    with_vec(g.v4, [&](auto v) {
      constexpr int VEC = decltype(v)::value;
      if constexpr (bn_built<VEC, TX>)
        hipLaunchKernelGGL((k_bn_stats<VEC, TX>), dim3(g.C, p.sp), dim3(256), 0, s, x, g.N, g.C, g.HWv,
                           p.sp, p.per, part);
    });
    tail(part, p.sp);
  } else {
    tail(nullptr, 1);
  }
  return launch_status(fn);
}

// k_bn_apply over the apply grid: e2ep_bn_fwd's tail (scale / shift null) or e2ep_bn_apply
static void bn_launch_apply(const BnPlan &p, const float *x, const double *part, int sp,
                            const BnFwd &a, const float *scale, const float *shift, hipStream_t s) {
  const BnGeom &g = p.g;
  with_vec(g.v4, [&](auto v) {
    hipLaunchKernelGGL((k_bn_apply<decltype(v)::value>), dim3(g.C, p.apply_blocks), dim3(256), 0, s, x,
                       part, sp, g.per_c, a.eps, a.momentum, a.running_mean, a.running_var, a.mean,
                       a.invstd, a.gamma, a.beta, a.res, a.dc_rand, a.dc_keep, g.N, g.C, g.HWv,
                       p.apply_per, a.act, a.y, scale, shift, p.rev_fwd);
  });
}

// what the backward kernels share
struct BnBwd {
  const float *mean, *invstd, *gamma, *beta, *res, *dc_rand;
  float dc_keep;
  BnGate gt;
  int act, train;
  float *dres, *dgamma, *dbeta;
};

// k_bn_bwd_apply over the apply grid: the split backward's second pass (part, sp) or
// e2ep_bn_bwd_planes (planes)
static void bn_launch_bwd_apply(const BnPlan &p, int io, const void *x, const void *dy, void *dx,
                                const BnBwd &a, const double *part, int sp, const double *planes,
                                hipStream_t s) {
  const BnGeom &g = p.g;
  with_vec(g.v4, [&](auto v) {
    with_bn_io(io, x, dy, dx, [&](auto *xt, auto *dyt, auto *dxt) {
      constexpr int VEC = decltype(v)::value;
      using TX = elem_t<decltype(xt)>;
      using TD = elem_t<decltype(dyt)>;
      using TO = elem_t<decltype(dxt)>;
      if constexpr (bn_built<VEC, TX, TD, TO>)
        hipLaunchKernelGGL((k_bn_bwd_apply<VEC, TX, TD, TO>), dim3(g.C, p.apply_blocks), dim3(256), 0,
                           s, xt, dyt, a.mean, a.invstd, a.gamma, a.beta, a.res, a.dc_rand, a.dc_keep,
                           a.gt, part, sp, g.per_c, g.N, g.C, g.HWv, p.apply_per, a.act, a.train, dxt,
                           a.dres, a.dgamma, a.dbeta, planes, p.rev_apply);
    });
  });
}

}  // namespace e2ep

using namespace e2ep;

extern "C" {

size_t e2ep_bn_workspace(int N, int C, int H, int W) { return bn_plan(bn_geom(N, C, H, W)).workspace; }

// 0 also for N, C, H or W <= 0
int e2ep_bn_fwd_split(int N, int C, int H, int W) {
  const BnPlan p = bn_plan(bn_geom(N, C, H, W));
  return p.g.valid && !p.fwd.T;
}

int e2ep_bn_bwd_split(int N, int C, int H, int W) {
  const BnPlan p = bn_plan(bn_geom(N, C, H, W));
  return p.g.valid && !p.bwd.T;
}

int e2ep_bn_fwd(const float *x, const float *gamma, const float *beta, const float *res,
                const float *dc_rand, float dc_keep, float *running_mean, float *running_var,
                int N, int C, int H, int W, int train, float momentum, float eps, int act,
                float *mean, float *invstd, float *y, void *workspace, size_t workspace_bytes,
                void *stream) {
  const char *fn = "e2ep_bn_fwd";
  const BnPlan p = bn_plan(bn_geom(N, C, H, W));
  if (int e = bn_check(fn, p, train != 0, workspace, workspace_bytes)) return e;
  E2EP_REQUIRE(act >= 0 && act <= 2, E2EP_EINVAL, "e2ep_bn_fwd: act must be 0/1/2");
  E2EP_REQUIRE(train || (running_mean && running_var), E2EP_EINVAL,
               "e2ep_bn_fwd: eval needs running stats");
  E2EP_REQUIRE(!dc_rand || dc_keep > 0.f, E2EP_EINVAL, "e2ep_bn_fwd: drop-connect keep must be > 0");
  const BnFwd a{eps, momentum, running_mean, running_var, mean, invstd, gamma, beta, res, dc_rand,
                dc_keep, act, y, nullptr, nullptr};
  hipStream_t s = as_stream(stream);
  return bn_fwd_run(fn, p, x, train, a, workspace, s, [&](const double *part, int sp) {
    bn_launch_apply(p, x, part, sp, a, nullptr, nullptr, s);
  });
}

int e2ep_bn_stats(const void *x, const float *gamma, const float *beta, float *running_mean,
                  float *running_var, int N, int C, int H, int W, int train, float momentum,
                  float eps, float *mean, float *invstd, float *scale, float *shift,
                  void *workspace, size_t workspace_bytes, void *stream, int io) {
  const char *fn = "e2ep_bn_stats";
  const BnPlan p = bn_plan(bn_geom(N, C, H, W));
  E2EP_REQUIRE(io == 0 || (io == E2EP_IO_X_BF16 && p.g.HW % 4 == 0), E2EP_EINVAL,
               "e2ep_bn_stats: storage mask %d not supported (0 or X bf16, H*W %% 4 == 0)", io);
  if (int e = bn_check(fn, p, train != 0, workspace, workspace_bytes)) return e;
  E2EP_REQUIRE(train || (running_mean && running_var), E2EP_EINVAL,
               "e2ep_bn_stats: eval needs running stats");
  E2EP_REQUIRE(mean && invstd && scale && shift, E2EP_EINVAL, "e2ep_bn_stats: null output");
  const BnFwd a{eps, momentum, running_mean, running_var, mean, invstd, gamma, beta, nullptr, nullptr,
                1.f, 0, nullptr, scale, shift};
  hipStream_t s = as_stream(stream);
  auto tail = [&](const double *part, int sp) {
    hipLaunchKernelGGL(k_bn_finalize, dim3(C), dim3(256), 0, s, part, sp, p.g.per_c, eps, momentum,
                       running_mean, running_var, mean, invstd, gamma, beta, scale, shift);
  };
  if (io) return bn_fwd_run(fn, p, static_cast<const bf16_t *>(x), train, a, workspace, s, tail);
  return bn_fwd_run(fn, p, static_cast<const float *>(x), train, a, workspace, s, tail);
}

size_t e2ep_bn_finalize_part_workspace(int C, int tiles) {
  (void)C;
  (void)tiles;
  return 0;  // one launch, no workspace (kept in the ABI for a future split plan)
}

int e2ep_bn_finalize_part(const double *part, int tiles, const float *gamma, const float *beta,
                          float *running_mean, float *running_var, int N, int C, int H, int W,
                          float momentum, float eps, float *mean, float *invstd, float *scale,
                          float *shift, void *workspace, size_t workspace_bytes, void *stream) {
  const BnGeom g = bn_geom(N, C, H, W);
  E2EP_REQUIRE(part && tiles > 0 && g.valid && C <= 65535, E2EP_EINVAL,
               "e2ep_bn_finalize_part: bad arguments");
  E2EP_REQUIRE(mean && invstd && scale && shift, E2EP_EINVAL, "e2ep_bn_finalize_part: null output");
  E2EP_REQUIRE(!running_mean == !running_var, E2EP_EINVAL,
               "e2ep_bn_finalize_part: running_mean / running_var both or neither");
  (void)workspace;
  (void)workspace_bytes;
  hipLaunchKernelGGL(k_bn_finalize_tiles, dim3(cdiv(C, FT_CH)), dim3(FT_CH * FT_GROUPS), 0, as_stream(stream),
                     part, tiles, C, g.per_c, eps, momentum, running_mean, running_var, mean, invstd,
                     gamma, beta, scale, shift);
  return launch_status("e2ep_bn_finalize_part");
}

int e2ep_bn_apply(const float *x, const float *scale, const float *shift, const float *res,
                  const float *dc_rand, float dc_keep, int N, int C, int H, int W, int act,
                  float *y, void *stream) {
  const char *fn = "e2ep_bn_apply";
  const bool aligned = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)res) & 15) == 0;
  const BnPlan p = bn_plan(bn_geom(N, C, H, W, aligned));
  if (int e = bn_check(fn, p)) return e;
  E2EP_REQUIRE(x && y && scale && shift && act >= 0 && act <= 2, E2EP_EINVAL,
               "e2ep_bn_apply: bad arguments");
  E2EP_REQUIRE(!dc_rand || dc_keep > 0.f, E2EP_EINVAL, "e2ep_bn_apply: drop-connect keep must be > 0");
  const BnFwd a{0.f, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, res, dc_rand, dc_keep,
                act, y, nullptr, nullptr};
  bn_launch_apply(p, x, nullptr, 1, a, scale, shift, as_stream(stream));
  return launch_status(fn);
}

int e2ep_bn_bwd(const void *x, const void *dy, const float *mean, const float *invstd,
                const float *gamma, const float *beta, const float *res, const float *dc_rand,
                float dc_keep, const float *gate_logit, const float *gate_dpooled, int N, int C,
                int H, int W, int train, int act, void *dx, float *dgamma, float *dbeta,
                float *dres, void *workspace, size_t workspace_bytes, void *stream, int io) {
  const char *fn = "e2ep_bn_bwd";
  const BnPlan p = bn_plan(bn_geom(N, C, H, W));
  const BnGeom &g = p.g;
  if (int e = bn_check(fn, p)) return e;
  E2EP_REQUIRE(!gate_logit == !gate_dpooled, E2EP_EINVAL,
               "e2ep_bn_bwd: gate_logit / gate_dpooled both or neither");
  E2EP_REQUIRE(!dc_rand || dc_keep > 0.f, E2EP_EINVAL, "e2ep_bn_bwd: drop-connect keep must be > 0");
  E2EP_REQUIRE(bn_io_ok(io) && (io == 0 || g.HW % 4 == 0), E2EP_EINVAL,
               "e2ep_bn_bwd: storage mask %d not supported (0, X|DX, X|DY|DX or DY bf16, "
               "H*W %% 4 == 0)", io);
  const BnBwd a{mean, invstd, gamma, beta, res, dc_rand, dc_keep,
                BnGate{gate_logit, gate_dpooled, 1.f / (float)g.HW}, act, train, dres, dgamma, dbeta};
  hipStream_t s = as_stream(stream);
  if (p.bwd.T) {
    with_layout(p.bwd, [&](auto t, auto r) {
      with_bn_io(io, x, dy, dx, [&](auto *xt, auto *dyt, auto *dxt) {
        constexpr int T = decltype(t)::value;
        hipLaunchKernelGGL((k_bn_bwd_small<T, decltype(r)::value, elem_t<decltype(xt)>,
                                           elem_t<decltype(dyt)>, elem_t<decltype(dxt)>>),
                           dim3(g.C), dim3(T), 0, s, xt, dyt, a.mean, a.invstd, a.gamma, a.beta, a.res,
                           a.dc_rand, a.dc_keep, a.gt, g.per_c, g.N, g.C, g.HWv, a.act, a.train, dxt,
                           a.dres, a.dgamma, a.dbeta);
      });
    });
    return launch_status(fn);
  }
  if (int e = bn_check(fn, p, true, workspace, workspace_bytes)) return e;
  double *part = static_cast<double *>(workspace);
  with_vec(g.v4, [&](auto v) {
    with_bn_io(io, x, dy, dx, [&](auto *xt, auto *dyt, auto *) {
      constexpr int VEC = decltype(v)::value;
      using TX = elem_t<decltype(xt)>;
      using TD = elem_t<decltype(dyt)>;
      if constexpr (bn_built<VEC, TX, TD>)
        hipLaunchKernelGGL((k_bn_bwd_reduce<VEC, TX, TD>), dim3(g.C, p.sp), dim3(256), 0, s, xt, dyt,
                           a.mean, a.invstd, a.gamma, a.beta, a.res, a.dc_rand, a.dc_keep, a.gt, g.N,
                           g.C, g.HWv, p.sp, p.per, a.act, part, p.rev_reduce);
    });
  });
  if (dx || dres)
    bn_launch_bwd_apply(p, io, x, dy, dx, a, part, p.sp, nullptr, s);
  else if (dgamma || dbeta)
    hipLaunchKernelGGL(k_bn_bwd_finalize, dim3(g.C), dim3(256), 0, s, part, p.sp, dgamma, dbeta);
  return launch_status(fn);
}

int e2ep_bn_bwd_planes(const void *x, const void *dy, const float *mean, const float *invstd,
                       const float *gamma, const float *beta, const float *gate_logit,
                       const float *gate_dpooled, const double *plane_sums, int N, int C, int H,
                       int W, int act, void *dx, float *dgamma, float *dbeta, void *stream, int io) {
  const char *fn = "e2ep_bn_bwd_planes";
  const BnPlan p = bn_plan(bn_geom(N, C, H, W));
  if (int e = bn_check(fn, p)) return e;
  E2EP_REQUIRE(x && dy && mean && invstd && gate_logit && gate_dpooled && plane_sums && dx,
               E2EP_EINVAL, "e2ep_bn_bwd_planes: null argument");
  E2EP_REQUIRE(act >= 0 && act <= 2, E2EP_EINVAL, "e2ep_bn_bwd_planes: act must be 0/1/2");
  // (a bf16 mask needs H * W % 4 == 0, so it always runs VEC = 4)
  E2EP_REQUIRE((io == BNIO_F32 || io == BNIO_XDX || io == BNIO_ALL) && (io == 0 || p.g.HW % 4 == 0),
               E2EP_EINVAL, "e2ep_bn_bwd_planes: storage mask %d not supported (0, X|DX or X|DY|DX "
               "bf16, H*W %% 4 == 0)", io);
  const BnBwd a{mean, invstd, gamma, beta, nullptr, nullptr, 1.f,
                BnGate{gate_logit, gate_dpooled, 1.f / (float)p.g.HW}, act, 1, nullptr, dgamma, dbeta};
  bn_launch_bwd_apply(p, io, x, dy, dx, a, nullptr, 1, plane_sums, as_stream(stream));
  return launch_status(fn);
}

int e2ep_bn_eval_multi(const long long *table, int n, void *stream) {
  E2EP_REQUIRE(table && n > 0 && n <= 65535, E2EP_EINVAL, "e2ep_bn_eval_multi: bad table (n %d)", n);
  hipLaunchKernelGGL(k_bn_eval_multi, dim3(n), dim3(256), 0, as_stream(stream), table);
  return launch_status("e2ep_bn_eval_multi");
}

int e2ep_bn_small_limits(int fwd_max_vec, int bwd_max_vec) {
  if (fwd_max_vec >= 0) g_bns_fwd_max = std::min(fwd_max_vec, BNS_R * BNS_T);
  if (bwd_max_vec >= 0) g_bns_bwd_max = std::min(bwd_max_vec, BNS_R * BNS_T);
  return 0;
}

int e2ep_bn_small(int on) {
  const int prev = g_bn_small;
  if (on >= 0) g_bn_small = on ? 1 : 0;
  return prev;
}

int e2ep_act_fwd(const float *x, long long n, int act, float *y, void *stream) {
  E2EP_REQUIRE(n >= 0 && act >= 0 && act <= 2, E2EP_EINVAL, "e2ep_act_fwd: bad args");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_act_fwd, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, n, act, y);
  return launch_status("e2ep_act_fwd");
}

int e2ep_act_bwd(const float *x, const float *dy, long long n, int act, float *dx, void *stream) {
  E2EP_REQUIRE(n >= 0 && act >= 0 && act <= 2, E2EP_EINVAL, "e2ep_act_bwd: bad args");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_act_bwd, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, dy, n, act, dx);
  return launch_status("e2ep_act_bwd");
}

}  // extern "C"

