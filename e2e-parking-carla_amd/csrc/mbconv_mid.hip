// The middle of an MBConv block on 16x16 maps in one launch per direction, NCHW fp32, gfx950:
//   _bn0 -> swish -> depthwise KxK (stride 1, SAME) -> _bn1 -> swish -> SE squeeze
// (efficientnet-pytorch 0.7.1 MBConvBlock.forward, used through model/cam_encoder.py:69-73).
// Every value of this chain depends on its own channel alone (both BatchNorms' batch
// statistics, the depthwise filter, the SE plane means; in the backward every BN sum and the
// depthwise weight gradient), and one channel of a 16x16 stage is at most 8192 floats: what the
// single-launch BatchNorm kernels (bn.hip k_bn_fwd_small / k_bn_bwd_small) hold in registers.
// So one workgroup per channel runs the whole chain, reading and writing each tensor once:
// forward reads y0 and writes y1 (instead of 5 tensor passes in 4 launches), backward reads
// gy, y1, y0 and writes dx (instead of 9-10 passes in 3 launches).
//
// Layout: that of k_bn_fwd_small<T, R> — thread t holds float4 vectors t, t + T, ... of the
// channel, so wave w owns planes w, w + T/64, ... and lane l the float4 l of a plane (row l / 4,
// columns 4 (l % 4) ..), which is also the strip kernels' lane-to-output map on a 16-wide plane
// (dwconv.hip).  Each step repeats the arithmetic and the summation order of the kernel it
// replaces (named at the step), so every output is bitwise that of the separate launches.  The
// depthwise weight gradient repeats k_dw_wgrad_strip's one-split order (what channel counts of
// 512 and more get, the 16x16 stages' 672 / 960 among them); where that kernel would sum
// several split slabs per channel (fewer channels) the sums differ in order, not in terms.
#include "bns_layout.h"
#include "common.h"

// as bn.hip / dwconv.hip / se.hip: a*b + c fuses within one expression only, so the
// expressions copied from those files round as they do there
#pragma clang fp contract(on)

namespace e2ep {

namespace {

constexpr int MID_HW = 16;            // plane side
constexpr int MID_HWV = 64;           // float4 per plane: one per lane
constexpr int MID_PADL = 4;           // dwconv.hip DW_PADL
constexpr int MID_WP = MID_HW + 2 * MID_PADL;  // LDS row pitch (floats)

__device__ __forceinline__ float f4get(const float4 &v, int i) {
  return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}

// bn.hip wave_sum_d / block_sum2_t with the caller's LDS (a kernel reduces more than once)
__device__ __forceinline__ double mid_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int T>
__device__ __forceinline__ void mid_block_sum2(double &s, double &q, double *rs, double *rq) {
  constexpr int NW = T / 64;
  s = mid_wave_sum_d(s);
  q = mid_wave_sum_d(q);
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

// float offset of float4 vector t of channel c (bn.hip bns_off with HWv = 64)
__device__ __forceinline__ size_t mid_off(int t, int C, int c) {
  const int n = t >> 6, p = t & 63;
  return (((size_t)n * C + c) * MID_HWV + p) * 4;
}

// dwconv.hip dw_wave_sync: a wave stages and reads only its own LDS window
__device__ __forceinline__ void mid_wave_sync() {
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0); vmcnt / expcnt unconstrained
  __builtin_amdgcn_wave_barrier();
}

// one BatchNorm of the forward: parameters, running statistics, saved outputs
struct MidBnFwd {
  const float *gamma, *beta;
  float *running_mean, *running_var;
  float *mean, *invstd, *scale, *shift;
  float eps, momentum;
};

// k_bn_fwd_small's finalize: mean / invstd / folded scale and shift from the channel's fp64
// sums; thread 0 writes them and updates the running statistics
__device__ __forceinline__ void mid_bn_finalize(double s, double q, long long cnt,
                                                const MidBnFwd &b, int c, float &sc, float &sh) {
  const double m = s / (double)cnt;
  double var = q / (double)cnt - m * m;
  if (var < 0.0) var = 0.0;
  const float mu = (float)m, is = (float)(1.0 / sqrt(var + (double)b.eps));
  sc = is * (b.gamma ? b.gamma[c] : 1.f);
  sh = (b.beta ? b.beta[c] : 0.f) - mu * sc;
  if (threadIdx.x == 0) {
    b.mean[c] = mu;
    b.invstd[c] = is;
    b.scale[c] = sc;
    b.shift[c] = sh;
    if (b.running_mean) {
      const double unb = cnt > 1 ? var * (double)cnt / (double)(cnt - 1) : var;
      b.running_mean[c] = (float)((1.0 - b.momentum) * b.running_mean[c] + b.momentum * m);
      b.running_var[c] = (float)((1.0 - b.momentum) * b.running_var[c] + b.momentum * unb);
    }
  }
}

// the depthwise kernels' input transform (dwconv.hip dw_in, act = swish) = se.hip se_in
__device__ __forceinline__ float mid_bn_swish(float v, float sc, float sh) {
  const float z = v * sc + sh;
  return swish_f(z);
}

// swish'(z) (bn.hip act_bwd)
__device__ __forceinline__ float mid_swish_bwd(float z) {
  const float s = sigmoid_f(z);
  return s * (1.f + z * (1.f - s));
}

// bn.hip BnBwdElem::with_factor without residual and drop-connect, act = swish: xhat and the
// gradient at the BN output
__device__ __forceinline__ void mid_bn_bwd_elem(float xv, float dyv, float mu, float is, float g,
                                                float b, float &xh, float &dzb) {
  xh = (xv - mu) * is;
  const float zb = xh * g + b;
  dzb = dyv * mid_swish_bwd(zb + 0.f);
}

// A wave's LDS window of one plane: rows [-pad, 16 + pad) x columns [-4, 20), zero outside the
// plane.  The zeros are written once; a plane's 16 x 16 values overwrite the inside.
template <int K>
struct MidWin {
  static constexpr int PAD = (K - 1) / 2;
  static constexpr int IR = MID_HW + K - 1;
  static constexpr int FLOATS = IR * MID_WP;
  static constexpr int NV = 3 + K;              // window floats a lane reads per row
  static constexpr int OFF = (4 - PAD) & 3;     // dwconv.hip dw_off(pl)
  static __device__ __forceinline__ void clear(float *win, int lane) {
    for (int e = lane; e < FLOATS / 4; e += 64)
      reinterpret_cast<float4 *>(win)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  static __device__ __forceinline__ void put(float *win, int lane, float4 v) {
    const int ro = lane >> 2, ox0 = 4 * (lane & 3);
    *reinterpret_cast<float4 *>(win + (ro + PAD) * MID_WP + MID_PADL + ox0) = v;
  }
  // the lane's window row for tap row a (dwconv.hip dw_row<NV, OFF>: aligned b128 reads)
  static __device__ __forceinline__ void row(const float *win, int lane, int a, float (&v)[NV]) {
    const int ro = lane >> 2, ox0 = 4 * (lane & 3);
    const float4 *p = reinterpret_cast<const float4 *>(win + (ro + a) * MID_WP + ox0);
    float f[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float4 t = p[i];
      f[4 * i] = t.x;
      f[4 * i + 1] = t.y;
      f[4 * i + 2] = t.z;
      f[4 * i + 3] = t.w;
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = f[OFF + j];
  }
  // the strip kernels' correlation (dw_fwd_strip_body's tap order) of the staged plane
  // (FENCE: a scheduling fence per tap row, so one row of the window is in registers at a time)
  template <bool FENCE = false>
  static __device__ __forceinline__ void conv(const float *win, int lane, const float (&wr)[K * K],
                                              float (&o)[4]) {
    o[0] = o[1] = o[2] = o[3] = 0.f;
#pragma unroll
    for (int a = 0; a < K; ++a) {
      float v[NV];
      row(win, lane, a, v);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int b = 0; b < K; ++b) o[q] = __builtin_fmaf(wr[a * K + b], v[q + b], o[q]);
      if (FENCE) __builtin_amdgcn_sched_barrier(0);
    }
  }
};

}  // namespace

template <int K, int T, int R>
__global__ void __launch_bounds__(T, 4) k_mbconv_mid_fwd(
    const float *__restrict__ y0, const float *__restrict__ w, MidBnFwd b0, MidBnFwd b1,
    long long cnt, int N, int C, float *__restrict__ y1, float *__restrict__ pooled) {
  using Win = MidWin<K>;
  constexpr int NW = T / 64;
  __shared__ __attribute__((aligned(16))) float wins[NW][Win::FLOATS];
  __shared__ double rs0[NW], rq0[NW], rs1[NW], rq1[NW];
  const int c = blockIdx.x, tot = N * MID_HWV;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *win = wins[wave];
  float4 v[R];
#pragma unroll
  for (int u = 0; u < R; ++u) v[u] = ld4(y0 + mid_off(min((int)threadIdx.x + u * T, tot - 1), C, c));
  Win::clear(win, lane);
  float wr[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) wr[t] = w[c * K * K + t];
  // _bn0 statistics (k_bn_fwd_small)
  double s = 0.0, q = 0.0;
#pragma unroll
  for (int u = 0; u < R; ++u) {
    if ((int)threadIdx.x + u * T >= tot) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double d = f4get(v[u], i);
      s += d;
      q += d * d;
    }
  }
  mid_block_sum2<T>(s, q, rs0, rq0);
  float sc, sh;
  mid_bn_finalize(s, q, cnt, b0, c, sc, sh);
  // depthwise conv of swish(bn0(y0)), plane by plane (k_dw_fwd_strip)
  float o[R][4];
#pragma unroll
  for (int u = 0; u < R; ++u) {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[u][i] = 0.f;
  }
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int t = threadIdx.x + u * T;
    if (t >= tot) break;  // wave-uniform: a plane is one wave's 64 vectors
    Win::put(win, lane, make_float4(mid_bn_swish(v[u].x, sc, sh), mid_bn_swish(v[u].y, sc, sh),
                                    mid_bn_swish(v[u].z, sc, sh), mid_bn_swish(v[u].w, sc, sh)));
    mid_wave_sync();
    Win::conv(win, lane, wr, o[u]);
    st4(y1 + mid_off(t, C, c), make_float4(o[u][0], o[u][1], o[u][2], o[u][3]));
    mid_wave_sync();  // LDS reuse
  }
  // _bn1 statistics of y1 (k_bn_fwd_small)
  s = 0.0;
  q = 0.0;
#pragma unroll
  for (int u = 0; u < R; ++u) {
    if ((int)threadIdx.x + u * T >= tot) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double d = o[u][i];
      s += d;
      q += d * d;
    }
  }
  mid_block_sum2<T>(s, q, rs1, rq1);
  mid_bn_finalize(s, q, cnt, b1, c, sc, sh);
  // SE squeeze of swish(bn1(y1)) (k_se_squeeze / plane_sum: a wave per plane)
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int t = threadIdx.x + u * T;
    if (t >= tot) break;
    const float4 a = make_float4(mid_bn_swish(o[u][0], sc, sh), mid_bn_swish(o[u][1], sc, sh),
                                 mid_bn_swish(o[u][2], sc, sh), mid_bn_swish(o[u][3], sc, sh));
    float ps = 0.f;
    ps += (a.x + a.y) + (a.z + a.w);
    ps = wave_sum(ps);
    if (lane == 0) pooled[(size_t)(t >> 6) * C + c] = ps / (float)(MID_HW * MID_HW);
  }
}

// The backward's per-channel inputs: the saved statistics and parameters of both BatchNorms
struct MidBnBwd {
  const float *mean, *invstd, *gamma, *beta;
  float *dgamma, *dbeta;
};

template <int K, int T, int R>
__global__ void __launch_bounds__(T, 4) k_mbconv_mid_bwd(
    const float *__restrict__ gy, const float *__restrict__ gate_logit,
    const float *__restrict__ gate_dpooled, float inv_hw, const float *__restrict__ y1,
    const float *__restrict__ y0, const float *__restrict__ w, MidBnBwd b1, MidBnBwd b0,
    const float *__restrict__ scale0, const float *__restrict__ shift0, long long cnt, int N, int C,
    float *__restrict__ dx, float *__restrict__ dw) {
  using Win = MidWin<K>;
  constexpr int NW = T / 64, KK = K * K;
  // k5 with 4 planes per wave: left alone the scheduler hoists both windows' rows of a plane
  // (2 x 60 registers) over the 57 of the held tensors and the tap sums, and spills
  constexpr bool FENCE = K == 5 && R == 4;
  __shared__ __attribute__((aligned(16))) float wing[NW][Win::FLOATS];  // dy1 planes
  __shared__ __attribute__((aligned(16))) float wina[NW][Win::FLOATS];  // a0 planes
  __shared__ double rs1[NW], rq1[NW], rs0[NW], rq0[NW];
  __shared__ float red[4][KK];
  const int c = blockIdx.x, tot = N * MID_HWV;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *wg = wing[wave], *wa = wina[wave];
  // every load of the block in flight at once (bn.hip bns_factors): the gate's per-plane
  // factors, then the three tensors
  float gs[R], gd[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int n = min((int)threadIdx.x + u * T, tot - 1) >> 6;
    gs[u] = gate_logit[n * C + c];
    gd[u] = gate_dpooled[n * C + c];
  }
  float4 xv[R], dv[R], x0[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const size_t off = mid_off(min((int)threadIdx.x + u * T, tot - 1), C, c);
    xv[u] = ld4(y1 + off);
    dv[u] = ld4(gy + off);
    x0[u] = ld4(y0 + off);
  }
  Win::clear(wg, lane);
  Win::clear(wa, lane);
  float wr[KK];  // flipped: the stride-1 data gradient is the forward's correlation (FLIP)
#pragma unroll
  for (int t = 0; t < KK; ++t) wr[t] = w[c * KK + (KK - 1 - t)];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    gs[u] = sigmoid_f(gs[u]);  // = BnGate::coef
    gd[u] = gd[u] * inv_hw;
  }
  // _bn1 backward with the SE gate (k_bn_bwd_small)
  float g1[R][4];  // dzb, then the gradient at y1
  {
    const float mu = b1.mean[c], is = b1.invstd[c];
    const float g = b1.gamma ? b1.gamma[c] : 1.f, b = b1.beta ? b1.beta[c] : 0.f;
    float xh[R][4];
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int t = threadIdx.x + u * T;
      float s4 = 0.f, q4 = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        mid_bn_bwd_elem(f4get(xv[u], i), f4get(dv[u], i) * gs[u] + gd[u], mu, is, g, b, xh[u][i],
                        g1[u][i]);
        s4 += g1[u][i];
        q4 = __builtin_fmaf(g1[u][i], xh[u][i], q4);
      }
      if (t < tot) {
        s += s4;
        q += q4;
      }
    }
    mid_block_sum2<T>(s, q, rs1, rq1);
    if (threadIdx.x == 0) {
      if (b1.dbeta) b1.dbeta[c] = (float)s;
      if (b1.dgamma) b1.dgamma[c] = (float)q;
    }
    const float ms = (float)(s / (double)cnt), mq = (float)(q / (double)cnt);
    const float gis = g * is;
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) g1[u][i] = gis * (g1[u][i] - (ms + xh[u][i] * mq));
  }
  // depthwise data gradient (k_dw_bwd_pair's flipped strip forward over dy1) and weight
  // gradient (dw_wgrad_strip_body's taps over a0 = swish(bn0(y0)), recomputed), plane by plane
  const float sc0 = scale0[c], sh0 = shift0[c];
  float dt[R][4];
#pragma unroll
  for (int u = 0; u < R; ++u) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dt[u][i] = 0.f;
  }
  // a plane's K*K weight-gradient taps added to the lane's running sums, in
  // dw_wgrad_strip_body's order
  auto taps = [&](int u, float (&acc)[KK]) {
#pragma unroll
    for (int a = 0; a < K; ++a) {
      float v[Win::NV];
      Win::row(wa, lane, a, v);
#pragma unroll
      for (int b = 0; b < K; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[a * K + b] = __builtin_fmaf(g1[u][j], v[j + b], acc[a * K + b]);
      if (FENCE) __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto stage = [&](int u) {
    Win::put(wg, lane, make_float4(g1[u][0], g1[u][1], g1[u][2], g1[u][3]));
    Win::put(wa, lane, make_float4(mid_bn_swish(x0[u].x, sc0, sh0), mid_bn_swish(x0[u].y, sc0, sh0),
                                   mid_bn_swish(x0[u].z, sc0, sh0), mid_bn_swish(x0[u].w, sc0, sh0)));
  };
  // The weight gradient repeats the one-split k_dw_wgrad_strip (what the 16x16 stages' channel
  // counts get): its wave j of 4 runs one fma chain per lane and tap through planes j, j + 4,
  // j + 8, ..., then a wave sum, then (r0 + r1) + (r2 + r3).
  if constexpr (NW == 4) {  // wave j owns exactly that chain's planes: the sums stay in registers
    float acc[KK];
#pragma unroll
    for (int t = 0; t < KK; ++t) acc[t] = 0.f;
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int t = threadIdx.x + u * T;
      if (t >= tot) break;  // wave-uniform
      stage(u);
      mid_wave_sync();
      taps(u, acc);
      Win::template conv<FENCE>(wg, lane, wr, dt[u]);
      mid_wave_sync();  // LDS reuse
    }
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const float r = wave_sum(acc[t]);
      if (lane == 0) red[wave][t] = r;
    }
  } else {
    // 8 waves: chain j alternates between waves j (planes j, j + 8, ...) and j + 4 (planes j + 4,
    // j + 12, ...), so the lane sums travel through LDS: in each half step one half of the waves
    // continues its chains while the other half runs its planes' data gradient
    __shared__ float xacc[4][KK][64];
    const int half = wave >> 2;
    float *xa = &xacc[wave & 3][0][lane];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const bool valid = (int)threadIdx.x + u * T < tot;  // wave-uniform
      if (valid) stage(u);
      mid_wave_sync();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool first = u == 0 && h == 0;  // starts the chains (zeros even without a plane)
        if (half == h) {
          if (valid || first) {  // a tap row's K sums in registers at a time
#pragma unroll
            for (int a = 0; a < K; ++a) {
              float acc[K], v[Win::NV];
#pragma unroll
              for (int b = 0; b < K; ++b) acc[b] = first ? 0.f : xa[(a * K + b) * 64];
              if (valid) {
                Win::row(wa, lane, a, v);
#pragma unroll
                for (int b = 0; b < K; ++b)
#pragma unroll
                  for (int j = 0; j < 4; ++j) acc[b] = __builtin_fmaf(g1[u][j], v[j + b], acc[b]);
              }
#pragma unroll
              for (int b = 0; b < K; ++b) xa[(a * K + b) * 64] = acc[b];
              if (FENCE) __builtin_amdgcn_sched_barrier(0);
            }
          }
        } else if (valid) {
          Win::template conv<FENCE>(wg, lane, wr, dt[u]);
        }
        __syncthreads();  // hands the sums to the other half; also orders the windows' reuse
      }
    }
    if (wave < 4) {
#pragma unroll
      for (int t = 0; t < KK; ++t) {
        const float r = wave_sum(xa[t * 64]);
        if (lane == 0) red[wave][t] = r;
      }
    }
  }
  // _bn0 backward (k_bn_bwd_small, no gate: its factors are 1 and 0)
  {
    const float mu = b0.mean[c], is = b0.invstd[c];
    const float g = b0.gamma ? b0.gamma[c] : 1.f, b = b0.beta ? b0.beta[c] : 0.f;
    float dzb[R][4];
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int t = threadIdx.x + u * T;
      float s4 = 0.f, q4 = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float xh;
        mid_bn_bwd_elem(f4get(x0[u], i), dt[u][i] * 1.f + 0.f, mu, is, g, b, xh, dzb[u][i]);
        s4 += dzb[u][i];
        q4 = __builtin_fmaf(dzb[u][i], xh, q4);
      }
      if (t < tot) {
        s += s4;
        q += q4;
      }
    }
    mid_block_sum2<T>(s, q, rs0, rq0);  // its barrier also publishes red[][]
    if (threadIdx.x == 0) {
      if (b0.dbeta) b0.dbeta[c] = (float)s;
      if (b0.dgamma) b0.dgamma[c] = (float)q;
    }
    if (threadIdx.x < KK) {
      const int t = threadIdx.x;
      dw[c * KK + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    }
    const float ms = (float)(s / (double)cnt), mq = (float)(q / (double)cnt);
    const float gis = g * is;
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int t = threadIdx.x + u * T;
      if (t >= tot) break;
      float ox[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float xh = (f4get(x0[u], i) - mu) * is;  // as mid_bn_bwd_elem (held there, redone here)
        ox[i] = gis * (dzb[u][i] - (ms + xh * mq));
      }
      st4(dx + mid_off(t, C, c), make_float4(ox[0], ox[1], ox[2], ox[3]));
    }
  }
}

// The <threads, vectors per thread> layout e2ep_bn_fwd / e2ep_bn_bwd give a channel of totv
// float4 (bns_layout.h), so the sums here run in their order: {0, 0} = none taken (the channel
// is too large, or 8 vectors on 256 threads, which these kernels do not build)
static BnsLayout mid_layout(int totv) {
  const BnsLayout l = bns_layout(totv);
  return l.R == BNS_R ? BnsLayout{0, 0} : l;
}

}  // namespace e2ep

using namespace e2ep;

#define MID_LAUNCH_K(KERNEL, KV, ...)                                                              \
  do {                                                                                             \
    if (T == 256 && R == 1) hipLaunchKernelGGL((KERNEL<KV, 256, 1>), dim3(C), dim3(256), 0, s, __VA_ARGS__); \
    else if (T == 256 && R == 2) hipLaunchKernelGGL((KERNEL<KV, 256, 2>), dim3(C), dim3(256), 0, s, __VA_ARGS__); \
    else if (T == 256) hipLaunchKernelGGL((KERNEL<KV, 256, 4>), dim3(C), dim3(256), 0, s, __VA_ARGS__); \
    else if (R == 1) hipLaunchKernelGGL((KERNEL<KV, 512, 1>), dim3(C), dim3(512), 0, s, __VA_ARGS__); \
    else if (R == 2) hipLaunchKernelGGL((KERNEL<KV, 512, 2>), dim3(C), dim3(512), 0, s, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<KV, 512, 4>), dim3(C), dim3(512), 0, s, __VA_ARGS__);          \
  } while (0)
#define MID_LAUNCH(KERNEL, ...)                        \
  do {                                                 \
    if (K == 3) MID_LAUNCH_K(KERNEL, 3, __VA_ARGS__);  \
    else MID_LAUNCH_K(KERNEL, 5, __VA_ARGS__);         \
  } while (0)

extern "C" {

// dims[10] = {N, C, H, W, K, P, Q, stride, pad_top, pad_left} (as the depthwise entry points)
int e2ep_mbconv_mid_ok(const int *d) {
  if (!d || g_tune[TUNE_MBCONV_MID] != 2) return 0;
  const int N = d[0], C = d[1], K = d[4];
  if (!(N > 0 && C > 0 && C <= 65535)) return 0;
  if (!(d[2] == MID_HW && d[3] == MID_HW && d[5] == MID_HW && d[6] == MID_HW && d[7] == 1)) return 0;
  if (!((K == 3 || K == 5) && d[8] == (K - 1) / 2 && d[9] == (K - 1) / 2)) return 0;
  if ((long long)N * MID_HW * MID_HW > 8192) return 0;
  // the separate launches must be the single-launch BatchNorm kernels, whose order this repeats
  if (e2ep_bn_fwd_split(N, C, MID_HW, MID_HW) || e2ep_bn_bwd_split(N, C, MID_HW, MID_HW)) return 0;
  return mid_layout(N * MID_HWV).T ? 1 : 0;
}

int e2ep_mbconv_mid_fwd(const float *y0, const float *w, const int *dims, const float *gamma0,
                        const float *beta0, float *running_mean0, float *running_var0,
                        float momentum0, float eps0, float *stats0, const float *gamma1,
                        const float *beta1, float *running_mean1, float *running_var1,
                        float momentum1, float eps1, float *stats1, float *y1, float *pooled,
                        void *stream) {
  E2EP_REQUIRE(e2ep_mbconv_mid_ok(dims) == 1, E2EP_EINVAL,
               "e2ep_mbconv_mid_fwd: shape not taken (e2ep_mbconv_mid_ok: 16x16 maps, stride 1, "
               "k 3|5 SAME, N*256 <= 8192, e2ep_tune key 36 = 2)");
  E2EP_REQUIRE(y0 && w && stats0 && stats1 && y1 && pooled, E2EP_EINVAL,
               "e2ep_mbconv_mid_fwd: null argument");
  E2EP_REQUIRE(!running_mean0 == !running_var0 && !running_mean1 == !running_var1, E2EP_EINVAL,
               "e2ep_mbconv_mid_fwd: running_mean / running_var both or neither");
  const int N = dims[0], C = dims[1], K = dims[4];
  const BnsLayout l = mid_layout(N * MID_HWV);
  const int T = l.T, R = l.R;
  const MidBnFwd b0{gamma0, beta0, running_mean0, running_var0, stats0, stats0 + C, stats0 + 2 * C,
                    stats0 + 3 * C, eps0, momentum0};
  const MidBnFwd b1{gamma1, beta1, running_mean1, running_var1, stats1, stats1 + C, stats1 + 2 * C,
                    stats1 + 3 * C, eps1, momentum1};
  hipStream_t s = as_stream(stream);
  const long long cnt = (long long)N * MID_HW * MID_HW;
  MID_LAUNCH(k_mbconv_mid_fwd, y0, w, b0, b1, cnt, N, C, y1, pooled);
  return launch_status("e2ep_mbconv_mid_fwd");
}

int e2ep_mbconv_mid_bwd(const float *gy, const float *gate_logit, const float *gate_dpooled,
                        const float *y1, const float *y0, const float *w, const int *dims,
                        const float *stats1, const float *gamma1, const float *beta1,
                        const float *stats0, const float *gamma0, const float *beta0, float *dx,
                        float *dgamma1, float *dbeta1, float *dgamma0, float *dbeta0, float *dw,
                        void *stream) {
  E2EP_REQUIRE(e2ep_mbconv_mid_ok(dims) == 1, E2EP_EINVAL,
               "e2ep_mbconv_mid_bwd: shape not taken (e2ep_mbconv_mid_ok: 16x16 maps, stride 1, "
               "k 3|5 SAME, N*256 <= 8192, e2ep_tune key 36 = 2)");
  E2EP_REQUIRE(gy && gate_logit && gate_dpooled && y1 && y0 && w && stats1 && stats0 && dx && dw,
               E2EP_EINVAL, "e2ep_mbconv_mid_bwd: null argument");
  const int N = dims[0], C = dims[1], K = dims[4];
  const BnsLayout l = mid_layout(N * MID_HWV);
  const int T = l.T, R = l.R;
  const MidBnBwd b1{stats1, stats1 + C, gamma1, beta1, dgamma1, dbeta1};
  const MidBnBwd b0{stats0, stats0 + C, gamma0, beta0, dgamma0, dbeta0};
  hipStream_t s = as_stream(stream);
  const long long cnt = (long long)N * MID_HW * MID_HW;
  MID_LAUNCH(k_mbconv_mid_bwd, gy, gate_logit, gate_dpooled, 1.f / (float)(MID_HW * MID_HW), y1, y0,
             w, b1, b0, stats0 + 2 * C, stats0 + 3 * C, cnt, N, C, dx, dw);
  return launch_status("e2ep_mbconv_mid_bwd");
}

}  // extern "C"
