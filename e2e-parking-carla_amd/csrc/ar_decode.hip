// Incremental (KV-cached) decoding of the control-token transformer decoder: one new position
// t per sample and step instead of the full (B, T) pass of reference
// model/control_predict.py:60-75.  The torch decoder layers are post-norm with ReLU,
//   x1 = LN1(x + SA(x));  x2 = LN2(x1 + CA(x1, mem));  x3 = LN3(x2 + FF(x2)),
// and a step runs six launches per layer on M = B <= 16 rows:
//   1 k_dec_self_attn   (sample, head): row -> this head's q, k, v; k, v into the layer's cache
//                       at position t; softmax(q K^T) V over the cached positions 0..t
//   2 k_dec_row_gemv    out-projection + residual
//   3 k_dec_cross_attn  (sample, head): row -> q; softmax(q K^T) V over the memory K|V that was
//                       projected once per predict
//   4 k_dec_row_gemv    out-projection + residual
//   5 k_dec_row_gemv    FFN1 + ReLU
//   6 k_dec_row_gemv    FFN2 + residual
// No launch exists only to normalise: the rows in memory are the pre-norm sums, and every
// consumer applies the LayerNorm as it loads the row (two wave reductions over E values).
// Layer 0's row is gathered, embedding[seq[b][t]] + pos_embed[t] (the clamp of
// k_embed_tokens_fwd), and written out once for the residual of launch 2.
//
// Every reduction runs in a fixed order (lanes stride k, xor-butterfly wave sums, partials
// combined in index order), there are no atomics and no workgroup reads what another of the
// same launch wrote, so a captured replay is bitwise an eager run.  fp32 FMA arithmetic.
// Rows are read with float2 loads when every row is 8-byte aligned (E = 258), else dword loads.
#include <math.h>

#include "common.h"

namespace e2ep {

constexpr int DEC_MAXB = 16, DEC_MAXT = 32, DEC_MAXDH = 64, DEC_MAXSK = 256;
constexpr int DEC_MAXK = 4088;  // row length: DEC_RB staged rows + their statistics in 64 KiB of LDS
constexpr int DEC_KS = DEC_MAXDH + 1;  // LDS row stride of a staged K / V tile (odd: no conflicts)
constexpr int DEC_CK = 128;            // memory keys staged per pass of the cross attention
constexpr int DEC_RB = 4;              // rows per workgroup of the row GEMV (one wave stages each)
constexpr int DEC_TH = 1024;           // threads of an attention workgroup
constexpr int DEC_R = 4;               // projection rows a wave has in flight at once
constexpr int DEC_U = 4;               // weight loads a wave of the row GEMV has in flight

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// LayerNorm statistics of one row by one wave (torch: biased variance, two passes)
__device__ __forceinline__ void row_stats(const float *__restrict__ row, int n, float eps, int lane,
                                          float &mean, float &rstd) {
  float s = 0.f;
  for (int k = lane; k < n; k += 64) s += row[k];
  mean = wave_sum(s) / (float)n;
  float q = 0.f;
  for (int k = lane; k < n; k += 64) {
    const float d = row[k] - mean;
    q = fmaf(d, d, q);
  }
  rstd = 1.f / sqrtf(wave_sum(q) / (float)n + eps);
}

// R dot products sum_k w[r][k] xs[k] by one wave at once (w global, xs LDS): the R rows' loads
// are independent, so they are in flight together (a wave that took its rows one by one waited
// out one memory latency per row).  V = 2 needs K even and every row 8-byte aligned.
template <int V, int R>
__device__ __forceinline__ void wave_dots(const float *const (&w)[R], const float *xs, int K,
                                          int lane, float (&acc)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  if (V == 2) {
    for (int k = 2 * lane; k < K; k += 128) {
      const float2 x = *reinterpret_cast<const float2 *>(xs + k);
      float2 a[R];
#pragma unroll
      for (int r = 0; r < R; ++r) a[r] = *reinterpret_cast<const float2 *>(w[r] + k);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        acc[r] = fmaf(a[r].x, x.x, acc[r]);
        acc[r] = fmaf(a[r].y, x.y, acc[r]);
      }
    }
  } else {
    for (int k = lane; k < K; k += 64) {
      const float x = xs[k];
      float a[R];
#pragma unroll
      for (int r = 0; r < R; ++r) a[r] = w[r][k];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = fmaf(a[r], x, acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
}

// The whole workgroup stages LN(row) (or the row itself when gamma is null) into xs[0..E).
// Each wave computes the statistics itself (the same values in every wave).
__device__ __forceinline__ void stage_row(const float *__restrict__ row, int E,
                                          const float *__restrict__ gamma,
                                          const float *__restrict__ beta, float eps, float *xs) {
  const int tid = threadIdx.x, lane = tid & 63;
  if (gamma) {
    float mean, rstd;
    row_stats(row, E, eps, lane, mean, rstd);
    for (int e = tid; e < E; e += blockDim.x)
      xs[e] = fmaf((row[e] - mean) * rstd, gamma[e], beta ? beta[e] : 0.f);
  } else {
    for (int e = tid; e < E; e += blockDim.x) xs[e] = row[e];
  }
}

struct DecSelfArgs {
  const float *x;  // (B, ldx) pre-norm rows, or null: gather from table / pos
  int ldx;
  const float *gamma, *beta;
  float eps;
  const float *table;  // (V, E)
  int V;
  const float *pos;  // (T, E)
  float *x0;         // (B, E): the gathered row (written when x is null)
  const int64_t *seq;
  int seq_stride;
  int64_t pad;
  const float *w_in, *b_in;  // (3E, E), (3E) or null
  float *cache;              // (B, T, 2, E)
  float *out;                // (B, E)
  int T, t, E, H, dh;
  float scale;
};

// grid (H, B), block DEC_TH (16 waves: the 3 dh projection rows of a head are the kernel's
// time, and a workgroup is all a (sample, head) has).  LDS: xs[Ep] | q[64] | k[32][65] |
// v[32][65] | p[32]
template <int V>
__global__ void __launch_bounds__(DEC_TH) k_dec_self_attn(const DecSelfArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Ep = (a.E + 3) & ~3;
  float *xs = smem, *qs = xs + Ep, *ks = qs + DEC_MAXDH, *vs = ks + DEC_MAXT * DEC_KS,
        *ps = vs + DEC_MAXT * DEC_KS;
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = a.E, dh = a.dh, t = a.t, c0 = h * dh;
  float *cache = a.cache + (size_t)b * a.T * 2 * E;
  // cached k, v of the positions before t (written by earlier launches)
  for (int i = tid; i < t * dh; i += DEC_TH) {
    const int j = i / dh, d = i - j * dh;
    ks[j * DEC_KS + d] = cache[(size_t)(2 * j) * E + c0 + d];
    vs[j * DEC_KS + d] = cache[(size_t)(2 * j + 1) * E + c0 + d];
  }
  if (a.x) {
    stage_row(a.x + (size_t)b * a.ldx, E, a.gamma, a.beta, a.eps, xs);
  } else {
    int64_t v = a.seq[(size_t)b * a.seq_stride + t];
    v = v < 0 ? 0 : (v >= a.V ? a.V - 1 : v);  // never read out of the table
    for (int e = tid; e < E; e += DEC_TH) {
      const float r = a.table[(size_t)v * E + e] + a.pos[(size_t)t * E + e];
      xs[e] = r;
      if (h == 0) a.x0[(size_t)b * E + e] = r;
    }
  }
  __syncthreads();
  // this head's q, k, v rows of the packed in-projection: DEC_R outputs per wave at a time
  // (output i: row (i / dh) * E + c0 + i % dh; the tail repeats the last row and drops it)
  const int nout = 3 * dh;
  for (int i0 = wave * DEC_R; i0 < nout; i0 += (DEC_TH / 64) * DEC_R) {
    const float *w[DEC_R];
    int n[DEC_R];
#pragma unroll
    for (int r = 0; r < DEC_R; ++r) {
      const int i = min(i0 + r, nout - 1), which = i / dh;
      n[r] = which * E + c0 + i - which * dh;
      w[r] = a.w_in + (size_t)n[r] * E;
    }
    float acc[DEC_R];
    wave_dots<V, DEC_R>(w, xs, E, lane, acc);
#pragma unroll
    for (int r = 0; r < DEC_R; ++r) {
      if (lane != r || i0 + r >= nout) continue;
      const int which = (i0 + r) / dh, d = i0 + r - which * dh;
      const float v = acc[r] + (a.b_in ? a.b_in[n[r]] : 0.f);
      if (which == 0) {
        qs[d] = v * a.scale;
      } else {
        (which == 1 ? ks : vs)[t * DEC_KS + d] = v;
        cache[(size_t)(2 * t + which - 1) * E + c0 + d] = v;
      }
    }
  }
  __syncthreads();
  if (wave == 0) {  // scores and softmax over the keys 0..t (t < 32): one lane per key
    const bool live = lane <= t && a.seq[(size_t)b * a.seq_stride + lane] != a.pad;
    float s = -INFINITY;
    if (live) {
      s = 0.f;
      for (int d = 0; d < dh; ++d) s = fmaf(qs[d], ks[lane * DEC_KS + d], s);
    }
    const float m = wave_max(s);
    const float e = live ? expf(s - m) : 0.f;
    const float l = wave_sum(e);
    if (lane < DEC_MAXT) ps[lane] = l > 0.f ? e / l : 0.f;  // every key masked: zeros
  }
  __syncthreads();
  if (tid < dh) {
    float o = 0.f;
    for (int j = 0; j <= t; ++j) o = fmaf(ps[j], vs[j * DEC_KS + tid], o);
    a.out[(size_t)b * E + c0 + tid] = o;
  }
}

struct DecCrossArgs {
  const float *x;  // (B, ldx) pre-norm rows
  int ldx;
  const float *gamma, *beta;
  float eps;
  const float *w_q, *b_q;  // (E, E), (E) or null
  const float *kv;         // (B, Sk, ldkv): K at column 0, V at column E
  int ldkv;
  float *out;  // (B, E)
  int Sk, E, H, dh;
  float scale;
};

// grid (H, B), block DEC_TH.  LDS: xs[Ep] | q[64] | k[128][65] | p[256] | red[8] | part[16][64]
template <int V>
__global__ void __launch_bounds__(DEC_TH) k_dec_cross_attn(const DecCrossArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NW = DEC_TH / 64;
  const int Ep = (a.E + 3) & ~3;
  float *xs = smem, *qs = xs + Ep, *kt = qs + DEC_MAXDH, *ps = kt + DEC_CK * DEC_KS,
        *red = ps + DEC_MAXSK, *part = red + 8;
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = a.E, dh = a.dh, Sk = a.Sk, c0 = h * dh;
  const float *kv = a.kv + (size_t)b * Sk * a.ldkv + c0;
  stage_row(a.x + (size_t)b * a.ldx, E, a.gamma, a.beta, a.eps, xs);
  __syncthreads();
  for (int d0 = wave * DEC_R; d0 < dh; d0 += NW * DEC_R) {  // the head's q, DEC_R rows per wave
    const float *w[DEC_R];
#pragma unroll
    for (int r = 0; r < DEC_R; ++r) w[r] = a.w_q + (size_t)(c0 + min(d0 + r, dh - 1)) * E;
    float acc[DEC_R];
    wave_dots<V, DEC_R>(w, xs, E, lane, acc);
#pragma unroll
    for (int r = 0; r < DEC_R; ++r)
      if (lane == r && d0 + r < dh)
        qs[d0 + r] = (acc[r] + (a.b_q ? a.b_q[c0 + d0 + r] : 0.f)) * a.scale;
  }
  // scores: the head's K columns staged DEC_CK keys at a time (lanes run along d: each key's
  // dh values are contiguous), then one thread per key
  for (int j0 = 0; j0 < Sk; j0 += DEC_CK) {
    const int nk = min(DEC_CK, Sk - j0);
    __syncthreads();  // qs written / the previous tile read
#pragma unroll 2
    for (int i = tid; i < nk * dh; i += DEC_TH) {
      const int j = i / dh, d = i - j * dh;
      kt[j * DEC_KS + d] = kv[(size_t)(j0 + j) * a.ldkv + d];
    }
    __syncthreads();
    if (tid < nk) {
      float s = 0.f;
      for (int d = 0; d < dh; ++d) s = fmaf(qs[d], kt[tid * DEC_KS + d], s);
      ps[j0 + tid] = s;
    }
  }
  __syncthreads();
  // softmax over the Sk <= 256 scores, one per thread of the first four waves
  const float s = tid < Sk ? ps[tid] : -INFINITY;
  float m = wave_max(s);
  if (lane == 0 && wave < 4) red[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float e = tid < Sk ? expf(s - m) : 0.f;
  const float ws = wave_sum(e);
  if (lane == 0 && wave < 4) red[4 + wave] = ws;
  __syncthreads();
  const float l = (red[4] + red[5]) + (red[6] + red[7]);
  if (tid < Sk) ps[tid] = e / l;
  __syncthreads();
  // P V: wave g sums the keys g, g + NW, ... in order, lane d one output column; the NW
  // partial sums are added in wave order
  float acc = 0.f;
  if (lane < dh) {
    const float *vcol = kv + E + lane;
#pragma unroll 4
    for (int j = wave; j < Sk; j += NW) acc = fmaf(ps[j], vcol[(size_t)j * a.ldkv], acc);
  }
  part[wave * 64 + lane] = acc;
  __syncthreads();
  if (tid < dh) {
    float o = 0.f;
#pragma unroll
    for (int g = 0; g < NW; ++g) o += part[g * 64 + tid];
    a.out[(size_t)b * E + c0 + tid] = o;
  }
}

struct DecGemvArgs {
  const float *x;  // (B, ldx)
  int ldx;
  const float *gamma, *beta;  // LayerNorm of x on load (null: none)
  float eps;
  const float *w, *bias;  // (N, K), (N) or null
  const float *res;       // (B, ldr) residual (null: none)
  int ldr;
  const float *rgamma, *rbeta;  // LayerNorm of the residual row on load (null: none)
  float reps;
  float *out;  // (B, ldo)
  int ldo, B, N, K, relu;
};

// out[b][n] = act(sum_k LN?(x[b])[k] w[n][k] + bias[n]) + LN?(res[b])[n]
// grid (ceil(N / 4), ceil(B / DEC_RB)), block 256: wave r stages row b0 + r, then each wave
// owns one output column for the DEC_RB rows.  LDS: xs[DEC_RB][Kp] | rstat[DEC_RB][2]
template <int V>
__global__ void __launch_bounds__(256) k_dec_row_gemv(const DecGemvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K = a.K, Kp = (K + 3) & ~3;
  float *xs = smem, *rstat = xs + DEC_RB * Kp;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.y * DEC_RB, nr = min(DEC_RB, a.B - b0);
  const int n = blockIdx.x * 4 + wave;
  const float *wrow = a.w + (size_t)min(n, a.N - 1) * K;
  // the wave's first DEC_U weight loads are issued ahead of the staging (they do not depend on
  // it); every later trip of the k loop has DEC_U loads in flight as well
  float2 w0[DEC_U];
  if (V == 2) {
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const int k = 2 * lane + 128 * u;
      w0[u] = k < K ? *reinterpret_cast<const float2 *>(wrow + k) : make_float2(0.f, 0.f);
    }
  }
  if (wave < nr) {
    const float *row = a.x + (size_t)(b0 + wave) * a.ldx;
    float *xr = xs + wave * Kp;
    if (a.gamma) {
      float mean, rstd;
      row_stats(row, K, a.eps, lane, mean, rstd);
      for (int k = lane; k < K; k += 64)
        xr[k] = fmaf((row[k] - mean) * rstd, a.gamma[k], a.beta ? a.beta[k] : 0.f);
    } else {
      for (int k = lane; k < K; k += 64) xr[k] = row[k];
    }
    if (a.res && a.rgamma) {
      float mean, rstd;
      row_stats(a.res + (size_t)(b0 + wave) * a.ldr, a.N, a.reps, lane, mean, rstd);
      if (lane == 0) {
        rstat[2 * wave] = mean;
        rstat[2 * wave + 1] = rstd;
      }
    }
  }
  __syncthreads();
  if (n >= a.N) return;
  float acc[DEC_RB] = {0.f, 0.f, 0.f, 0.f};
  if (V == 2) {
    for (int k0 = 2 * lane; k0 < K; k0 += 128 * DEC_U) {
      float2 wv[DEC_U];
#pragma unroll
      for (int u = 0; u < DEC_U; ++u) {
        const int k = k0 + 128 * u;
        wv[u] = k0 == 2 * lane ? w0[u]
                : k < K        ? *reinterpret_cast<const float2 *>(wrow + k)
                               : make_float2(0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < DEC_U; ++u) {
        const int k = k0 + 128 * u;
        if (k >= K) break;
#pragma unroll
        for (int r = 0; r < DEC_RB; ++r) {
          if (r < nr) {
            const float2 x = *reinterpret_cast<const float2 *>(xs + r * Kp + k);
            acc[r] = fmaf(wv[u].x, x.x, acc[r]);
            acc[r] = fmaf(wv[u].y, x.y, acc[r]);
          }
        }
      }
    }
  } else {
#pragma unroll 4
    for (int k = lane; k < K; k += 64) {
      const float wv = wrow[k];
#pragma unroll
      for (int r = 0; r < DEC_RB; ++r)
        if (r < nr) acc[r] = fmaf(wv, xs[r * Kp + k], acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < DEC_RB; ++r) {
    if (r >= nr) break;
    float v = wave_sum(acc[r]);
    if (lane != r) continue;
    if (a.bias) v += a.bias[n];
    if (a.relu) v = fmaxf(v, 0.f);
    if (a.res) {
      float x = a.res[(size_t)(b0 + r) * a.ldr + n];
      if (a.rgamma)
        x = fmaf((x - rstat[2 * r]) * rstat[2 * r + 1], a.rgamma[n], a.rbeta ? a.rbeta[n] : 0.f);
      v += x;
    }
    a.out[(size_t)(b0 + r) * a.ldo + n] = v;
  }
}

static bool al8(const void *p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace e2ep

using namespace e2ep;

extern "C" {

int e2ep_dec_self_attn(const float *x, int ldx, const float *gamma, const float *beta, float eps,
                       const float *table, int V, const float *pos, float *x0, const int64_t *seq,
                       int seq_stride, int64_t pad, const float *w_in, const float *b_in,
                       float *cache, float *out, int B, int T, int t, int E, int H, void *stream) {
  E2EP_REQUIRE(seq && w_in && cache && out && B > 0 && T > 0 && E > 0 && H > 0 && E % H == 0 &&
                   t >= 0 && seq_stride >= T,
               E2EP_EINVAL, "e2ep_dec_self_attn: bad arguments");
  E2EP_REQUIRE(x ? ldx >= E : (table && pos && x0 && V > 0), E2EP_EINVAL,
               "e2ep_dec_self_attn: needs the input rows (ldx >= E), or table, pos and x0");
  const int dh = E / H;
  E2EP_REQUIRE(B <= DEC_MAXB && T <= DEC_MAXT && dh <= DEC_MAXDH && E <= DEC_MAXK, E2EP_ERANGE,
               "e2ep_dec_self_attn: B %d T %d head dim %d E %d (limits %d, %d, %d, %d)", B, T, dh,
               E, DEC_MAXB, DEC_MAXT, DEC_MAXDH, DEC_MAXK);
  E2EP_REQUIRE(t < T, E2EP_EINVAL, "e2ep_dec_self_attn: position %d outside 0 .. %d", t, T - 1);
  const DecSelfArgs a{x, ldx, gamma, beta, eps, table, V, pos, x0, seq, seq_stride, pad, w_in, b_in,
                      cache, out, T, t, E, H, dh, 1.f / sqrtf((float)dh)};
  const size_t lds = sizeof(float) * (((E + 3) & ~3) + DEC_MAXDH + 2 * DEC_MAXT * DEC_KS + DEC_MAXT);
  if (E % 2 == 0 && al8(w_in))
    hipLaunchKernelGGL(k_dec_self_attn<2>, dim3(H, B), dim3(DEC_TH), lds, as_stream(stream), a);
  else
    hipLaunchKernelGGL(k_dec_self_attn<1>, dim3(H, B), dim3(DEC_TH), lds, as_stream(stream), a);
  return launch_status("e2ep_dec_self_attn");
}

int e2ep_dec_cross_attn(const float *x, int ldx, const float *gamma, const float *beta, float eps,
                        const float *w_q, const float *b_q, const float *kv, int ldkv, float *out,
                        int B, int Sk, int E, int H, void *stream) {
  E2EP_REQUIRE(x && w_q && kv && out && B > 0 && Sk > 0 && E > 0 && H > 0 && E % H == 0 &&
                   ldx >= E && ldkv >= 2 * E,
               E2EP_EINVAL, "e2ep_dec_cross_attn: bad arguments");
  const int dh = E / H;
  E2EP_REQUIRE(B <= DEC_MAXB && Sk <= DEC_MAXSK && dh <= DEC_MAXDH && E <= DEC_MAXK, E2EP_ERANGE,
               "e2ep_dec_cross_attn: B %d Sk %d head dim %d E %d (limits %d, %d, %d, %d)", B, Sk,
               dh, E, DEC_MAXB, DEC_MAXSK, DEC_MAXDH, DEC_MAXK);
  const DecCrossArgs a{x, ldx, gamma, beta, eps, w_q, b_q, kv, ldkv, out, Sk, E, H, dh,
                       1.f / sqrtf((float)dh)};
  const size_t lds = sizeof(float) * (((E + 3) & ~3) + DEC_MAXDH + DEC_CK * DEC_KS + DEC_MAXSK + 8 + DEC_TH);
  if (E % 2 == 0 && al8(w_q))
    hipLaunchKernelGGL(k_dec_cross_attn<2>, dim3(H, B), dim3(DEC_TH), lds, as_stream(stream), a);
  else
    hipLaunchKernelGGL(k_dec_cross_attn<1>, dim3(H, B), dim3(DEC_TH), lds, as_stream(stream), a);
  return launch_status("e2ep_dec_cross_attn");
}

int e2ep_dec_row_gemv(const float *x, int ldx, const float *gamma, const float *beta, float eps,
                      const float *w, const float *bias, const float *res, int ldr,
                      const float *res_gamma, const float *res_beta, float res_eps, float *out,
                      int ldo, int B, int N, int K, int relu, void *stream) {
  E2EP_REQUIRE(x && w && out && B > 0 && N > 0 && K > 0 && ldx >= K && ldo >= N &&
                   (!res || ldr >= N),
               E2EP_EINVAL, "e2ep_dec_row_gemv: bad arguments");
  E2EP_REQUIRE(B <= DEC_MAXB && K <= DEC_MAXK, E2EP_ERANGE,
               "e2ep_dec_row_gemv: B %d K %d (limits %d, %d)", B, K, DEC_MAXB, DEC_MAXK);
  const DecGemvArgs a{x, ldx, gamma, beta, eps, w, bias, res, ldr, res_gamma, res_beta, res_eps,
                      out, ldo, B, N, K, relu};
  const size_t lds = sizeof(float) * (DEC_RB * ((K + 3) & ~3) + 2 * DEC_RB);
  const dim3 grid(cdiv(N, 4), cdiv(B, DEC_RB));
  if (K % 2 == 0 && al8(w))
    hipLaunchKernelGGL(k_dec_row_gemv<2>, grid, dim3(256), lds, as_stream(stream), a);
  else
    hipLaunchKernelGGL(k_dec_row_gemv<1>, grid, dim3(256), lds, as_stream(stream), a);
  return launch_status("e2ep_dec_row_gemv");
}

}  // extern "C"
