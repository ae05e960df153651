// Parameter-gradient finishing kernels, shared by their own launches (conv.hip, ln.hip, se.hip)
// and the deferred, batched launches of pgrad.hip.
//
// The split-K slab sum of a conv weight gradient, the LayerNorm dgamma / dbeta partial sum and
// the squeeze-excitation weight gradient produce parameter gradients only: nothing reads them
// before the optimizer (or the gradient gather) after the backward, yet each is a 5-8 us launch
// between two kernels of the activation-gradient chain.  Inside a deferral scope
// (e2ep_defer_begin .. e2ep_defer_flush) their call sites record their arguments instead of
// launching, and the flush runs one batched kernel per kind.  A block of a batched kernel runs
// the same device function below as a block of the kernel it replaces, so every output is
// summed in the same order and the results are equal bit for bit.
#pragma once
#include "common.h"

namespace e2ep {

// ---- the per-block bodies ------------------------------------------------------------------

// Fixed-order sum of the split slabs (+ optional accumulate into an existing gradient).
// Block = 64 outputs x 16 split lanes (1024 threads): thread (o, r) sums splits r, r+16, ...
// with 4 independent chains, then the 16 lane sums are added in order through LDS.
// Entries i whose tap (i % RS) is not live in `mask` are never written by the GEMM: their
// result is 0 (a weight tap that only ever meets zero padding).  blk: the block's index.
__device__ __forceinline__ void reduce_splits_block(const float *__restrict__ part, int splits, int n,
                                                    float *__restrict__ out, int accumulate, int RS,
                                                    unsigned long long mask, int blk,
                                                    float (*red)[64]) {
  const int o = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int i = blk * 64 + o;
  const bool live = (mask >> (i % RS)) & 1ULL;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < n && live) {
    int k = r;
    for (; k + 48 < splits; k += 64) {
      s0 += part[(size_t)(k + 0) * n + i];
      s1 += part[(size_t)(k + 16) * n + i];
      s2 += part[(size_t)(k + 32) * n + i];
      s3 += part[(size_t)(k + 48) * n + i];
    }
    for (; k < splits; k += 16) s0 += part[(size_t)k * n + i];
  }
  red[r][o] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (r == 0 && i < n) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += red[j][o];
    out[i] = accumulate ? out[i] + s : s;
  }
}

// The same reduction, four consecutive outputs i .. i+3 per thread (n % 4 == 0, i < n): float4
// loads of every slab in split order, summed in that order.  The 16-lane tree above runs ~1.4
// loads per thread and left the launch latency-bound (15 us for the 13.5 MB of slabs of a 16x16
// 1x1 conv's weight gradient, ~1 TB/s); here each thread keeps all its slab loads in flight.
__device__ __forceinline__ void reduce_splits4_thread(const float *__restrict__ part, int splits,
                                                      int n, float *__restrict__ out,
                                                      int accumulate, int RS,
                                                      unsigned long long mask, int i) {
  float4 acc = *reinterpret_cast<const float4 *>(part + i);
#pragma unroll 8
  for (int k = 1; k < splits; ++k) {
    const float4 v = *reinterpret_cast<const float4 *>(part + (size_t)k * n + i);
    acc.x += v.x;
    acc.y += v.y;
    acc.z += v.z;
    acc.w += v.w;
  }
  float r[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (!((mask >> ((i + e) % RS)) & 1ULL)) r[e] = 0.f;  // dead tap: never written by the GEMM
  float4 o = make_float4(r[0], r[1], r[2], r[3]);
  if (accumulate) {
    const float4 a = *reinterpret_cast<const float4 *>(out + i);
    o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
  }
  *reinterpret_cast<float4 *>(out + i) = o;
}

// LayerNorm dgamma / dbeta = fixed-order sums of the per-block partials: block = 64 columns x
// 16 partial lanes (1024 threads; thread (c, r) takes blocks r, r+16, ...), lanes added in
// order via LDS.  bx: the block's column group, by: 0 gamma, 1 beta.
__device__ __forceinline__ void ln_param_grads_block(const float *__restrict__ part, int nblk, int E,
                                                     float *__restrict__ dgamma,
                                                     float *__restrict__ dbeta, int bx, int by,
                                                     float (*red)[64]) {
  const int o = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int c = bx * 64 + o;
  const float *pp = part + (size_t)by * nblk * E;
  float s = 0.f;
  if (c < E)
    for (int k = r; k < nblk; k += 16) s += pp[(size_t)k * E + c];
  red[r][o] = s;
  __syncthreads();
  if (r == 0 && c < E) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) t += red[j][o];
    float *out = by == 0 ? dgamma : dbeta;
    if (out) out[c] = t;
  }
}

// Squeeze-excitation weight gradients, sums over the batch in sample order (output i per thread):
//   dW1[k][c] = sum_n dhpre[n][k] pooled[n][c]     dW2[c][k] = sum_n da[n][c] swish(hpre[n][k])
//   db1[k]    = sum_n dhpre[n][k]                  db2[c]    = sum_n da[n][c]
__device__ __forceinline__ void se_wgrad_thread(const float *__restrict__ pooled,
                                                const float *__restrict__ hpre,
                                                const float *__restrict__ da,
                                                const float *__restrict__ dhpre, int N, int C, int sq,
                                                float *__restrict__ dw1, float *__restrict__ db1,
                                                float *__restrict__ dw2, float *__restrict__ db2,
                                                int i) {
  const int n1 = sq * C, n2 = C * sq;
  float s = 0.f;
  if (i < n1) {
    const int k = i / C, c = i - k * C;
#pragma unroll 8
    for (int n = 0; n < N; ++n) s += dhpre[(size_t)n * sq + k] * pooled[(size_t)n * C + c];
    if (dw1) dw1[i] = s;
  } else if (i < n1 + n2) {
    const int j = i - n1, c = j / sq, k = j - c * sq;
#pragma unroll 8
    for (int n = 0; n < N; ++n) {
      const float z = hpre[(size_t)n * sq + k];
      s += da[(size_t)n * C + c] * (z * sigmoid_f(z));
    }
    if (dw2) dw2[j] = s;
  } else if (i < n1 + n2 + sq) {
    const int k = i - n1 - n2;
#pragma unroll 8
    for (int n = 0; n < N; ++n) s += dhpre[(size_t)n * sq + k];
    if (db1) db1[k] = s;
  } else if (i < n1 + n2 + sq + C) {
    const int c = i - n1 - n2 - sq;
#pragma unroll 8
    for (int n = 0; n < N; ++n) s += da[(size_t)n * C + c];
    if (db2) db2[c] = s;
  }
}

// ---- deferral records (pgrad.hip) -----------------------------------------------------------

// What one call site would have launched, with every argument by value.
struct SlabRec {  // reduce_splits (conv.hip)
  const float *part;
  float *out;
  unsigned long long mask;
  int n, splits, RS;
  int flags;  // bit 0: accumulate; bit 1: the float4 flavour (reduce_splits' choice)
};
struct LnRec {  // k_ln_param_grads (ln.hip)
  const float *part;
  float *dgamma, *dbeta;
  int nblk, E;
};
struct SeRec {  // k_se_wgrad (se.hip)
  const float *pooled, *hpre, *da, *dhpre;
  float *dw1, *db1, *dw2, *db2;
  int N, C, sq;
};

// True when the record was taken (a scope is open, not held, and e2ep_tune key 37 defers this
// kind): the caller then skips its launch.  False: the caller launches as without a scope.
bool pgrad_defer(const SlabRec &r);
bool pgrad_defer(const LnRec &r);
bool pgrad_defer(const SeRec &r);

}  // namespace e2ep
