// Fused Adam (torch.optim.Adam semantics, L2 weight decay, no amsgrad) over ONE flat fp32
// parameter buffer — the optimizer the reference configures at trainer/pl_trainer.py:116-121.
//
// Parameters, exp_avg and exp_avg_sq are flat, every tensor 16-byte aligned inside them; the
// gradients are either the per-tensor buffers autograd produced (a device table of pointers,
// so no accumulate-into-flat copy is needed) or one flat buffer (data-parallel: gathered and
// all-reduced).  One launch updates all ~28M weights: 7 x 4 bytes per weight of HBM traffic.
//
// Optional (e2ep_adam_step_clipped): global gradient-norm clipping and skipping of a non-finite
// step.  k_gnorm_partial (one fp64 sum of squares per chunk-table row) -> k_gnorm_final (one
// workgroup: norm, clip coefficient, skip flag, all left in device memory) -> k_adam_clip, which
// reads the coefficient and the flag there: one capturable chain, no host synchronisation, no
// atomics, the same bits whatever the gradient source or its alignment.  k_grad_accum adds a
// micro-step's gradients into the flat buffer (gradient accumulation).
//
// Optional (e2ep_adam_step_ema): an exponential moving average of the weights, a fourth flat
// buffer in the parameter layout, updated by the Adam launch itself while the new weight is
// still in a register: 9 x 4 bytes per weight instead of 7 x 4, no second pass.  k_flat_swap
// exchanges the contents of two flat buffers (evaluate with the averaged weights: every
// parameter keeps its address, so captured graphs see the swap).
//
// Optional (e2ep_adam_step_groups): parameter groups.  The chunk-table row's fourth int is its
// tensor's group; the launch reads that group's learning rate, weight decay and flags (bit 0:
// decoupled, AdamW's p *= 1 - lr * wd in place of the L2 term g += wd * p) from three device
// tables.  Still one launch and 7 x 4 bytes per weight (9 x 4 with the average); the gradient
// norm, the clip coefficient, the step counter and the average stay global.  k_adam_groups is
// adam_row with GROUPS set: the same expressions in the same order, so a grouped step gives the
// bits of the ungrouped one where the hyper-parameters agree.
#include "common.h"

namespace e2ep {

// torch.optim.Adam evaluates its scalars in double on the host and hands them to fp32
// kernels: beta**step and lr/bc1 in double, (1 - beta) in double then rounded to fp32.
// The learning rate is read from device memory (a double written by the host when an LR
// scheduler changes it), so a captured step follows CosineAnnealingLR under graph replay.
struct AdamHyper {
  double beta1, beta2;
  float b1f, b2f, w1, w2, eps, wd, grad_scale;
};

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_VEC = 4;
constexpr int ADAM_ITERS = 4;

__global__ void k_adam_count(float *step) { step[0] += 1.f; }

// The update of one chunk-table row {tensor, start element within tensor, length, group}.
// GROUPS: the row's learning rate, weight decay and flags come from the group tables at c.w
// (block-uniform); a row whose group is outside [0, n_groups) is left untouched and never
// indexes them.  Without GROUPS c.w is not read: lr[0] and h.wd hold for every row.
// CLIP: the gradient is also multiplied by a clip coefficient read from device memory (after
// grad_scale, before the weight decay), for the launch that follows k_gnorm_final.
// EMA: after an element's new p is known, ema = ema + ew * (p - ema), formed as ONE fp32 fused
// multiply-add fmaf(ew, p - ema, ema) (the subtraction rounds, the multiply-add rounds once);
// written as __fmaf_rn so that the vector path, its scalar tail and the unaligned-gradient
// path give the same bits whatever the compiler's contraction setting.  A row whose tensor has
// no gradient keeps p, m, v and `stepped` and still averages toward the unchanged p
// (torch.optim.swa_utils.AveragedModel.update_parameters); with ema == p, as it is from
// construction for a tensor that is never stepped, that is the identity (ew * 0 + ema).
__device__ __forceinline__ float ema_upd(float ev, float pv, float ew) {
  return __fmaf_rn(ew, pv - ev, ev);
}

template <bool CLIP, bool EMA = false, bool GROUPS = false>
__device__ __forceinline__ void adam_row(const int4 *__restrict__ chunks,
                                         const long long *__restrict__ offs,
                                         const long long *__restrict__ gptrs,
                                         const float *__restrict__ gflat, float *__restrict__ p,
                                         float *__restrict__ m, float *__restrict__ v,
                                         const float *__restrict__ step,
                                         const double *__restrict__ lr, const AdamHyper &h,
                                         float coef, int *__restrict__ stepped,
                                         float *__restrict__ ema = nullptr, float ew = 0.f,
                                         const double *__restrict__ group_wd = nullptr,
                                         const int *__restrict__ group_flags = nullptr,
                                         int n_groups = 0) {
  const int4 c = chunks[blockIdx.x];
  if (GROUPS && (unsigned)c.w >= (unsigned)n_groups) return;  // block-uniform
  const long long off = offs[c.x] + c.y;
  // a parameter without a gradient this step is not stepped (as torch.optim.Adam); on the
  // flat (all-reduced) path the table still says which parameters had one, so the result
  // does not depend on the world size
  const float *gt = gptrs ? reinterpret_cast<const float *>(gptrs[c.x]) : nullptr;
  if (gptrs && gt == nullptr) {  // block-uniform
    if (EMA) {  // p and ema rows are 16-byte aligned by the layout
      const float *pp = p + off;
      float *ep = ema + off;
#pragma unroll
      for (int it = 0; it < ADAM_ITERS; ++it) {
        const int i = (it * ADAM_THREADS + threadIdx.x) * ADAM_VEC;
        if (i >= c.z) break;
        if (i + ADAM_VEC <= c.z) {
          const float4 P = *reinterpret_cast<const float4 *>(pp + i);
          float4 E = *reinterpret_cast<const float4 *>(ep + i);
          E.x = ema_upd(E.x, P.x, ew);
          E.y = ema_upd(E.y, P.y, ew);
          E.z = ema_upd(E.z, P.z, ew);
          E.w = ema_upd(E.w, P.w, ew);
          *reinterpret_cast<float4 *>(ep + i) = E;
        } else {
          for (int j = i; j < c.z; ++j) ep[j] = ema_upd(ep[j], pp[j], ew);
        }
      }
    }
    return;
  }
  // per-tensor "stepped at least once" flag (torch.optim.Adam keeps state only for those)
  if (stepped && c.y == 0 && threadIdx.x == 0) stepped[c.x] = 1;
  const float *g = gflat ? gflat + off : gt + c.y;
  // torch: bias_correction = 1 - beta**step (python double), step_size = lr / bc1,
  // denom = sqrt(v) / sqrt(bc2) + eps, p -= step_size * m / denom
  const double t = (double)step[0];
  const double bc1 = 1.0 - pow(h.beta1, t);
  const double bc2 = 1.0 - pow(h.beta2, t);
  const double lrv = GROUPS ? lr[c.w] : lr[0];
  const float step_size = (float)(lrv / bc1);
  // L2 (torch.optim.Adam): g += wd * p.  Decoupled (AdamW): p *= 1 - lr * wd first, the
  // product and the difference in double as torch forms them on the host, and no L2 term.
  const bool decoupled = GROUPS && (group_flags[c.w] & 1) != 0;
  const float wd = GROUPS ? (float)group_wd[c.w] : h.wd;
  const float keep = decoupled ? (float)(1.0 - lrv * group_wd[c.w]) : 1.f;
  const float bc2s = (float)sqrt(bc2);
  const float w1 = h.w1, w2 = h.w2;
  float *pp = p + off, *mp = m + off, *vp = v + off;
  float *ep = EMA ? ema + off : nullptr;
  const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;  // wave-uniform
  auto upd = [&](float &pv, float &mv, float &vv, float gv) {
    if (GROUPS && decoupled) pv = pv * keep;
    gv = gv * h.grad_scale;
    if (CLIP) gv = gv * coef;  // clip_grad_norm_: g.mul_(clip_coef), then Adam's g + wd * p
    if (!(GROUPS && decoupled)) gv = gv + wd * pv;
    mv = mv + w1 * (gv - mv);  // exp_avg.lerp_(grad, 1 - beta1)
    vv = vv * h.b2f + w2 * gv * gv;
    const float den = sqrtf(vv) / bc2s + h.eps;
    pv = pv - step_size * (mv / den);
  };
  if (vec) {
#pragma unroll
    for (int it = 0; it < ADAM_ITERS; ++it) {
      const int i = (it * ADAM_THREADS + threadIdx.x) * ADAM_VEC;
      if (i >= c.z) break;
      if (i + ADAM_VEC <= c.z) {
        float4 P = *reinterpret_cast<const float4 *>(pp + i);
        float4 M = *reinterpret_cast<const float4 *>(mp + i);
        float4 V = *reinterpret_cast<const float4 *>(vp + i);
        const float4 G = *reinterpret_cast<const float4 *>(g + i);
        float4 E;
        if (EMA) E = *reinterpret_cast<const float4 *>(ep + i);
        upd(P.x, M.x, V.x, G.x);
        upd(P.y, M.y, V.y, G.y);
        upd(P.z, M.z, V.z, G.z);
        upd(P.w, M.w, V.w, G.w);
        *reinterpret_cast<float4 *>(pp + i) = P;
        *reinterpret_cast<float4 *>(mp + i) = M;
        *reinterpret_cast<float4 *>(vp + i) = V;
        if (EMA) {
          E.x = ema_upd(E.x, P.x, ew);
          E.y = ema_upd(E.y, P.y, ew);
          E.z = ema_upd(E.z, P.z, ew);
          E.w = ema_upd(E.w, P.w, ew);
          *reinterpret_cast<float4 *>(ep + i) = E;
        }
      } else {
        for (int j = i; j < c.z; ++j) {
          upd(pp[j], mp[j], vp[j], g[j]);
          if (EMA) ep[j] = ema_upd(ep[j], pp[j], ew);
        }
      }
    }
  } else {
    for (int j = threadIdx.x; j < c.z; j += ADAM_THREADS) {
      upd(pp[j], mp[j], vp[j], g[j]);
      if (EMA) ep[j] = ema_upd(ep[j], pp[j], ew);
    }
  }
}

__global__ void __launch_bounds__(ADAM_THREADS)
    k_adam(const int4 *__restrict__ chunks, const long long *__restrict__ offs,
           const long long *__restrict__ gptrs, const float *__restrict__ gflat,
           float *__restrict__ p, float *__restrict__ m, float *__restrict__ v,
           const float *__restrict__ step, const double *__restrict__ lr, AdamHyper h,
           int *__restrict__ stepped) {
  adam_row<false>(chunks, offs, gptrs, gflat, p, m, v, step, lr, h, 1.f, stepped);
}

// ---- gradient norm, clip coefficient, skip flag (the launches in front of k_adam_clip) ----

// 256 per-thread fp64 values -> their sum in a fixed order: an xor butterfly inside each
// 64-lane wave (every lane ends with the same bits), then the four wave sums left to right.
__device__ __forceinline__ double block_sum_f64(double acc, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// One fp64 sum of squares per chunk-table row (0 for a tensor without a gradient).  Products
// and sums are fp64, so the sum is finite exactly when every value is.  Element j of the row
// always belongs to thread (j / 4) % 256 and is added in increasing j, whether the gradient is
// read with 16-byte loads or, from an unaligned address, one float at a time: the partial does
// not depend on the load width.
__global__ void __launch_bounds__(ADAM_THREADS)
    k_gnorm_partial(const int4 *__restrict__ chunks, const long long *__restrict__ offs,
                    const long long *__restrict__ gptrs, const float *__restrict__ gflat,
                    double *__restrict__ partial) {
  __shared__ double red[ADAM_THREADS / 64];
  const int4 c = chunks[blockIdx.x];
  const float *gt = gptrs ? reinterpret_cast<const float *>(gptrs[c.x]) : nullptr;
  if (gptrs && gt == nullptr) {  // block-uniform
    if (threadIdx.x == 0) partial[blockIdx.x] = 0.0;
    return;
  }
  const float *g = gflat ? gflat + offs[c.x] + c.y : gt + c.y;
  const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
  double acc = 0.0;
  auto add = [&](float gv) { acc = acc + (double)gv * (double)gv; };
#pragma unroll
  for (int it = 0; it < ADAM_ITERS; ++it) {
    const int i = (it * ADAM_THREADS + threadIdx.x) * ADAM_VEC;
    if (i >= c.z) break;
    if (vec && i + ADAM_VEC <= c.z) {
      const float4 G = *reinterpret_cast<const float4 *>(g + i);
      add(G.x);
      add(G.y);
      add(G.z);
      add(G.w);
    } else {
      const int e = min(i + ADAM_VEC, c.z);
      for (int j = i; j < e; ++j) add(g[j]);
    }
  }
  const double s = block_sum_f64(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One workgroup: thread t adds partials t, t + 256, ... in that order, then block_sum_f64.
// norm = sqrt(sum) * |grad_scale|; coef = max_norm / (norm + 1e-6) limited to 1 by a compare
// that lets a NaN through (torch.clamp(max=1.0)), or exactly 1 when max_norm < 0 (clipping
// off); skip = skip_nonfinite and the norm is not finite; skipped counts the skips.
__global__ void __launch_bounds__(ADAM_THREADS)
    k_gnorm_final(const double *__restrict__ partial, int n, double grad_scale, double max_norm,
                  int skip_nonfinite, double *__restrict__ norm, float *__restrict__ coef,
                  int *__restrict__ skip, long long *__restrict__ skipped) {
  __shared__ double red[ADAM_THREADS / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += ADAM_THREADS) acc = acc + partial[i];
  const double s = block_sum_f64(acc, red);
  if (threadIdx.x != 0) return;
  const double nrm = sqrt(s) * fabs(grad_scale);
  double cf = 1.0;
  if (max_norm >= 0.0) {
    cf = max_norm / (nrm + 1e-6);
    if (cf > 1.0) cf = 1.0;
  }
  const int sk = (skip_nonfinite && !isfinite(nrm)) ? 1 : 0;
  norm[0] = nrm;
  coef[0] = (float)cf;
  skip[0] = sk;
  skipped[0] += sk;
}

__global__ void k_adam_count_unless(float *step, const int *__restrict__ skip) {
  if (skip[0] == 0) step[0] += 1.f;
}

// k_adam with the clip coefficient; a set skip flag leaves parameters, moments and the
// stepped flags as they are
__global__ void __launch_bounds__(ADAM_THREADS)
    k_adam_clip(const int4 *__restrict__ chunks, const long long *__restrict__ offs,
                const long long *__restrict__ gptrs, const float *__restrict__ gflat,
                float *__restrict__ p, float *__restrict__ m, float *__restrict__ v,
                const float *__restrict__ step, const double *__restrict__ lr, AdamHyper h,
                const float *__restrict__ coef, const int *__restrict__ skip,
                int *__restrict__ stepped) {
  if (skip[0] != 0) return;
  adam_row<true>(chunks, offs, gptrs, gflat, p, m, v, step, lr, h, coef[0], stepped);
}

// ---- EMA shadow weights (e2ep_adam_step_ema) and the buffer swap ----

// the step counter and the EMA update counter move together; neither moves on a skipped step
__global__ void k_adam_count_ema(float *step, long long *ema_updates,
                                 const int *__restrict__ skip) {
  if (skip && skip[0] != 0) return;
  step[0] += 1.f;
  ema_updates[0] += 1;
}

// k_adam / k_adam_clip with the EMA epilogue.  The averaging weight is evaluated in double,
// like Adam's scalars: d_t = decay, or with warm-up min(decay, (1 + n) / (10 + n)) (timm's
// ModelEmaV2 warm-up) with n = ema_updates[0] after the count launch (1 on the first update);
// ew = (float)(1 - d_t).  coef / skip may be null (no clipping / no skip flag).
template <bool CLIP>
__global__ void __launch_bounds__(ADAM_THREADS)
    k_adam_ema(const int4 *__restrict__ chunks, const long long *__restrict__ offs,
               const long long *__restrict__ gptrs, const float *__restrict__ gflat,
               float *__restrict__ p, float *__restrict__ m, float *__restrict__ v,
               const float *__restrict__ step, const double *__restrict__ lr, AdamHyper h,
               const float *__restrict__ coef, const int *__restrict__ skip,
               int *__restrict__ stepped, float *__restrict__ ema,
               const long long *__restrict__ ema_updates, double decay, int warmup) {
  if (skip && skip[0] != 0) return;
  double d = decay;
  if (warmup) {
    const double n = (double)ema_updates[0];
    d = fmin(decay, (1.0 + n) / (10.0 + n));
  }
  const float ew = (float)(1.0 - d);
  adam_row<CLIP, true>(chunks, offs, gptrs, gflat, p, m, v, step, lr, h, CLIP ? coef[0] : 1.f,
                       stepped, ema, ew);
}

// ---- parameter groups (e2ep_adam_step_groups) ----

// k_adam / k_adam_clip / k_adam_ema in one: coef (CLIP), skip and ema (EMA) may be null.  `lr`
// is the per-group table here.
template <bool CLIP, bool EMA>
__global__ void __launch_bounds__(ADAM_THREADS)
    k_adam_groups(const int4 *__restrict__ chunks, const long long *__restrict__ offs,
                  const long long *__restrict__ gptrs, const float *__restrict__ gflat,
                  float *__restrict__ p, float *__restrict__ m, float *__restrict__ v,
                  const float *__restrict__ step, const double *__restrict__ group_lr,
                  const double *__restrict__ group_wd, const int *__restrict__ group_flags,
                  int n_groups, AdamHyper h, const float *__restrict__ coef,
                  const int *__restrict__ skip, int *__restrict__ stepped,
                  float *__restrict__ ema, const long long *__restrict__ ema_updates,
                  double decay, int warmup) {
  if (skip && skip[0] != 0) return;
  float ew = 0.f;
  if (EMA) {
    double d = decay;
    if (warmup) {
      const double n = (double)ema_updates[0];
      d = fmin(decay, (1.0 + n) / (10.0 + n));
    }
    ew = (float)(1.0 - d);
  }
  adam_row<CLIP, EMA, true>(chunks, offs, gptrs, gflat, p, m, v, step, group_lr, h,
                            CLIP ? coef[0] : 1.f, stepped, ema, ew, group_wd, group_flags,
                            n_groups);
}

// a[i] <-> b[i] over n4 float4s: 16-byte accesses, grid-stride (the grid is capped, see
// e2ep_flat_swap), each element read and written by one thread only
constexpr int SWAP_THREADS = 256;
constexpr int SWAP_MAX_BLOCKS = 2048;  // 256 CUs x 8 workgroups

__global__ void __launch_bounds__(SWAP_THREADS)
    k_flat_swap(float4 *__restrict__ a, float4 *__restrict__ b, long long n4) {
  const long long stride = (long long)gridDim.x * SWAP_THREADS;
  for (long long i = (long long)blockIdx.x * SWAP_THREADS + threadIdx.x; i < n4; i += stride) {
    const float4 A = a[i];
    const float4 B = b[i];
    a[i] = B;
    b[i] = A;
  }
}

// gather per-tensor gradients into the flat (aligned, zero-padded) buffer for all-reduce
__global__ void __launch_bounds__(ADAM_THREADS)
    k_grad_gather(const int4 *__restrict__ chunks, const long long *__restrict__ offs,
                  const long long *__restrict__ gptrs, float *__restrict__ flat) {
  const int4 c = chunks[blockIdx.x];
  const float *g = reinterpret_cast<const float *>(gptrs[c.x]);
  float *o = flat + offs[c.x] + c.y;
  for (int j = threadIdx.x; j < c.z; j += ADAM_THREADS) o[j] = g ? g[c.y + j] : 0.f;
}

// flat[off + j] += g[j] over the chunk table (gradient accumulation; a tensor without a
// gradient adds nothing).  One add per element, so the load width does not change the result.
__global__ void __launch_bounds__(ADAM_THREADS)
    k_grad_accum(const int4 *__restrict__ chunks, const long long *__restrict__ offs,
                 const long long *__restrict__ gptrs, float *__restrict__ flat) {
  const int4 c = chunks[blockIdx.x];
  const float *gt = reinterpret_cast<const float *>(gptrs[c.x]);
  if (gt == nullptr) return;
  const float *g = gt + c.y;
  float *o = flat + offs[c.x] + c.y;  // 16-byte aligned: offsets and row starts are multiples of 4
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
#pragma unroll
    for (int it = 0; it < ADAM_ITERS; ++it) {
      const int i = (it * ADAM_THREADS + threadIdx.x) * ADAM_VEC;
      if (i >= c.z) break;
      if (i + ADAM_VEC <= c.z) {
        float4 O = *reinterpret_cast<const float4 *>(o + i);
        const float4 G = *reinterpret_cast<const float4 *>(g + i);
        O.x += G.x;
        O.y += G.y;
        O.z += G.z;
        O.w += G.w;
        *reinterpret_cast<float4 *>(o + i) = O;
      } else {
        for (int j = i; j < c.z; ++j) o[j] += g[j];
      }
    }
  } else {
    for (int j = threadIdx.x; j < c.z; j += ADAM_THREADS) o[j] += g[j];
  }
}

}  // namespace e2ep

using namespace e2ep;

extern "C" {

int e2ep_adam_chunk_elems(void) { return ADAM_THREADS * ADAM_VEC * ADAM_ITERS; }

int e2ep_adam_step(const int *chunks, int n_chunks, const long long *offsets,
                   const long long *grad_ptrs, const float *grad_flat, float *param, float *exp_avg,
                   float *exp_avg_sq, float *step, const double *lr, double beta1, double beta2,
                   double eps, double weight_decay, float grad_scale, int *stepped,
                   void *stream) {
  E2EP_REQUIRE(n_chunks > 0 && chunks && offsets && param && exp_avg && exp_avg_sq && step && lr,
               E2EP_EINVAL, "e2ep_adam_step: null argument");
  E2EP_REQUIRE(grad_ptrs || grad_flat, E2EP_EINVAL, "e2ep_adam_step: no gradients");
  AdamHyper h{beta1, beta2, (float)beta1, (float)beta2, (float)(1.0 - beta1),
              (float)(1.0 - beta2), (float)eps, (float)weight_decay, grad_scale};
  hipLaunchKernelGGL(k_adam_count, dim3(1), dim3(1), 0, as_stream(stream), step);
  hipLaunchKernelGGL(k_adam, dim3(n_chunks), dim3(ADAM_THREADS), 0, as_stream(stream),
                     reinterpret_cast<const int4 *>(chunks), offsets, grad_ptrs, grad_flat, param,
                     exp_avg, exp_avg_sq, step, lr, h, stepped);
  return launch_status("e2ep_adam_step");
}

int e2ep_grad_gather(const int *chunks, int n_chunks, const long long *offsets,
                     const long long *grad_ptrs, float *grad_flat, void *stream) {
  E2EP_REQUIRE(n_chunks > 0 && chunks && offsets && grad_ptrs && grad_flat, E2EP_EINVAL,
               "e2ep_grad_gather: null argument");
  hipLaunchKernelGGL(k_grad_gather, dim3(n_chunks), dim3(ADAM_THREADS), 0, as_stream(stream),
                     reinterpret_cast<const int4 *>(chunks), offsets, grad_ptrs, grad_flat);
  return launch_status("e2ep_grad_gather");
}

int e2ep_grad_sqnorm(const int *chunks, int n_chunks, const long long *offsets,
                     const long long *grad_ptrs, const float *grad_flat, double *partials,
                     void *stream) {
  E2EP_REQUIRE(n_chunks > 0 && chunks && offsets && partials, E2EP_EINVAL,
               "e2ep_grad_sqnorm: null argument");
  E2EP_REQUIRE(grad_ptrs || grad_flat, E2EP_EINVAL, "e2ep_grad_sqnorm: no gradients");
  hipLaunchKernelGGL(k_gnorm_partial, dim3(n_chunks), dim3(ADAM_THREADS), 0, as_stream(stream),
                     reinterpret_cast<const int4 *>(chunks), offsets, grad_ptrs, grad_flat,
                     partials);
  return launch_status("e2ep_grad_sqnorm");
}

int e2ep_grad_norm_finalize(const double *partials, int n_chunks, float grad_scale,
                            double max_norm, int skip_nonfinite, double *norm, float *clip_coef,
                            int *skip, long long *skipped, void *stream) {
  E2EP_REQUIRE(n_chunks > 0 && partials && norm && clip_coef && skip && skipped, E2EP_EINVAL,
               "e2ep_grad_norm_finalize: null argument");
  E2EP_REQUIRE(max_norm == max_norm, E2EP_EINVAL, "e2ep_grad_norm_finalize: max_norm is NaN");
  hipLaunchKernelGGL(k_gnorm_final, dim3(1), dim3(ADAM_THREADS), 0, as_stream(stream), partials,
                     n_chunks, (double)grad_scale, max_norm, skip_nonfinite, norm, clip_coef, skip,
                     skipped);
  return launch_status("e2ep_grad_norm_finalize");
}

int e2ep_adam_step_clipped(const int *chunks, int n_chunks, const long long *offsets,
                           const long long *grad_ptrs, const float *grad_flat, float *param,
                           float *exp_avg, float *exp_avg_sq, float *step, const double *lr,
                           double beta1, double beta2, double eps, double weight_decay,
                           float grad_scale, const float *clip_coef, const int *skip,
                           int *stepped, void *stream) {
  E2EP_REQUIRE(n_chunks > 0 && chunks && offsets && param && exp_avg && exp_avg_sq && step && lr &&
                   clip_coef && skip,
               E2EP_EINVAL, "e2ep_adam_step_clipped: null argument");
  E2EP_REQUIRE(grad_ptrs || grad_flat, E2EP_EINVAL, "e2ep_adam_step_clipped: no gradients");
  AdamHyper h{beta1, beta2, (float)beta1, (float)beta2, (float)(1.0 - beta1),
              (float)(1.0 - beta2), (float)eps, (float)weight_decay, grad_scale};
  hipLaunchKernelGGL(k_adam_count_unless, dim3(1), dim3(1), 0, as_stream(stream), step, skip);
  hipLaunchKernelGGL(k_adam_clip, dim3(n_chunks), dim3(ADAM_THREADS), 0, as_stream(stream),
                     reinterpret_cast<const int4 *>(chunks), offsets, grad_ptrs, grad_flat, param,
                     exp_avg, exp_avg_sq, step, lr, h, clip_coef, skip, stepped);
  return launch_status("e2ep_adam_step_clipped");
}

int e2ep_adam_step_ema(const int *chunks, int n_chunks, const long long *offsets,
                       const long long *grad_ptrs, const float *grad_flat, float *param,
                       float *exp_avg, float *exp_avg_sq, float *step, const double *lr,
                       double beta1, double beta2, double eps, double weight_decay,
                       float grad_scale, const float *clip_coef, const int *skip, int *stepped,
                       float *ema, long long *ema_updates, double ema_decay, int ema_warmup,
                       void *stream) {
  E2EP_REQUIRE(n_chunks > 0 && chunks && offsets && param && exp_avg && exp_avg_sq && step && lr &&
                   ema && ema_updates,
               E2EP_EINVAL, "e2ep_adam_step_ema: null argument");
  E2EP_REQUIRE(grad_ptrs || grad_flat, E2EP_EINVAL, "e2ep_adam_step_ema: no gradients");
  E2EP_REQUIRE(ema_decay >= 0.0 && ema_decay < 1.0, E2EP_EINVAL,
               "e2ep_adam_step_ema: ema_decay must be in [0, 1)");
  E2EP_REQUIRE(ema != param && ema != exp_avg && ema != exp_avg_sq, E2EP_EINVAL,
               "e2ep_adam_step_ema: ema aliases another buffer");
  AdamHyper h{beta1, beta2, (float)beta1, (float)beta2, (float)(1.0 - beta1),
              (float)(1.0 - beta2), (float)eps, (float)weight_decay, grad_scale};
  hipLaunchKernelGGL(k_adam_count_ema, dim3(1), dim3(1), 0, as_stream(stream), step, ema_updates,
                     skip);
  auto kern = clip_coef ? k_adam_ema<true> : k_adam_ema<false>;
  hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(ADAM_THREADS), 0, as_stream(stream),
                     reinterpret_cast<const int4 *>(chunks), offsets, grad_ptrs, grad_flat, param,
                     exp_avg, exp_avg_sq, step, lr, h, clip_coef, skip, stepped, ema,
                     static_cast<const long long *>(ema_updates), ema_decay, ema_warmup);
  return launch_status("e2ep_adam_step_ema");
}

int e2ep_adam_step_groups(const int *chunks, int n_chunks, const long long *offsets,
                          const long long *grad_ptrs, const float *grad_flat, float *param,
                          float *exp_avg, float *exp_avg_sq, float *step, const double *group_lr,
                          const double *group_wd, const int *group_flags, int n_groups,
                          double beta1, double beta2, double eps, float grad_scale,
                          const float *clip_coef, const int *skip, int *stepped, float *ema,
                          long long *ema_updates, double ema_decay, int ema_warmup,
                          void *stream) {
  E2EP_REQUIRE(n_chunks > 0 && chunks && offsets && param && exp_avg && exp_avg_sq && step,
               E2EP_EINVAL, "e2ep_adam_step_groups: null argument");
  E2EP_REQUIRE(grad_ptrs || grad_flat, E2EP_EINVAL, "e2ep_adam_step_groups: no gradients");
  E2EP_REQUIRE(n_groups >= 1, E2EP_EINVAL, "e2ep_adam_step_groups: n_groups must be >= 1");
  E2EP_REQUIRE(group_lr && group_wd && group_flags, E2EP_EINVAL,
               "e2ep_adam_step_groups: null group table");
  E2EP_REQUIRE((ema == nullptr) == (ema_updates == nullptr), E2EP_EINVAL,
               "e2ep_adam_step_groups: ema and ema_updates go together");
  if (ema) {
    E2EP_REQUIRE(ema_decay >= 0.0 && ema_decay < 1.0, E2EP_EINVAL,
                 "e2ep_adam_step_groups: ema_decay must be in [0, 1)");
    E2EP_REQUIRE(ema != param && ema != exp_avg && ema != exp_avg_sq, E2EP_EINVAL,
                 "e2ep_adam_step_groups: ema aliases another buffer");
  }
  // the weight decay is per group: AdamHyper's wd is not read by the grouped kernel
  AdamHyper h{beta1, beta2, (float)beta1, (float)beta2, (float)(1.0 - beta1),
              (float)(1.0 - beta2), (float)eps, 0.f, grad_scale};
  if (ema)
    hipLaunchKernelGGL(k_adam_count_ema, dim3(1), dim3(1), 0, as_stream(stream), step,
                       ema_updates, skip);
  else if (skip)
    hipLaunchKernelGGL(k_adam_count_unless, dim3(1), dim3(1), 0, as_stream(stream), step, skip);
  else
    hipLaunchKernelGGL(k_adam_count, dim3(1), dim3(1), 0, as_stream(stream), step);
  auto kern = ema ? (clip_coef ? k_adam_groups<true, true> : k_adam_groups<false, true>)
                  : (clip_coef ? k_adam_groups<true, false> : k_adam_groups<false, false>);
  hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(ADAM_THREADS), 0, as_stream(stream),
                     reinterpret_cast<const int4 *>(chunks), offsets, grad_ptrs, grad_flat, param,
                     exp_avg, exp_avg_sq, step, group_lr, group_wd, group_flags, n_groups, h,
                     clip_coef, skip, stepped, ema, static_cast<const long long *>(ema_updates),
                     ema_decay, ema_warmup);
  return launch_status("e2ep_adam_step_groups");
}

int e2ep_flat_swap(float *a, float *b, long long n, void *stream) {
  E2EP_REQUIRE(a && b, E2EP_EINVAL, "e2ep_flat_swap: null argument");
  E2EP_REQUIRE(n > 0 && n % 4 == 0, E2EP_EINVAL,
               "e2ep_flat_swap: n must be a positive multiple of 4");
  E2EP_REQUIRE(a != b, E2EP_EINVAL, "e2ep_flat_swap: a and b are the same buffer");
  E2EP_REQUIRE(a + n <= b || b + n <= a, E2EP_EINVAL, "e2ep_flat_swap: a and b overlap");
  E2EP_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0,
               E2EP_EINVAL, "e2ep_flat_swap: buffers must be 16-byte aligned");
  const long long n4 = n / 4;
  const long long blocks = (n4 + SWAP_THREADS - 1) / SWAP_THREADS;
  const int grid = (int)(blocks < SWAP_MAX_BLOCKS ? blocks : SWAP_MAX_BLOCKS);
  hipLaunchKernelGGL(k_flat_swap, dim3(grid), dim3(SWAP_THREADS), 0, as_stream(stream),
                     reinterpret_cast<float4 *>(a), reinterpret_cast<float4 *>(b), n4);
  return launch_status("e2ep_flat_swap");
}

int e2ep_grad_accumulate(const int *chunks, int n_chunks, const long long *offsets,
                         const long long *grad_ptrs, float *grad_flat, void *stream) {
  E2EP_REQUIRE(n_chunks > 0 && chunks && offsets && grad_ptrs && grad_flat, E2EP_EINVAL,
               "e2ep_grad_accumulate: null argument");
  hipLaunchKernelGGL(k_grad_accum, dim3(n_chunks), dim3(ADAM_THREADS), 0, as_stream(stream),
                     reinterpret_cast<const int4 *>(chunks), offsets, grad_ptrs, grad_flat);
  return launch_status("e2ep_grad_accumulate");
}

}  // extern "C"
