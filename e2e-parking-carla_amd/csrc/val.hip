// The validation half of an epoch on the device (fp32 logits in, device scalars and integer
// counts out), replacing the reference's PyTorch op chains:
//   control metrics  loss/control_loss.py:45-75 (ControlValLoss.forward): three slices, three
//       softmaxes, two argmaxes, the Python detokenize loop behind a synchronising .tolist(),
//       two SmoothL1Loss, two partial sums, stack, .T and CrossEntropyLoss;
//   val_loss         trainer/pl_trainer.py:85-114 (validation_step): sum(d.values()) of the
//       four losses, logged per batch;
//   segmentation IoU the confusion matrix of the BEV head's per-pixel argmax (the class the
//       agent steers by: agent.hip), which the reference never reports.
// Kernels:
//   k_ctrl_val_rows   one wave per used row 3f + k of each sample (rows T-2 and T-1 are not
//       used).  k = 0 / 1: the argmax token in torch.argmax's order (argmax.h), detokenised,
//       SmoothL1 (beta 1) against gt_acc / gt_steer.  k = 2: the fp32 softmax, its mass below
//       and from `split`, and the 2-way cross entropy of that pair used as logits.
//   k_ctrl_val_final  one workgroup: the per-row values summed by index, the two means and
//       the reverse mean over its non-ignored rows (NaN when there is none, as torch).
//   k_seg_conf_partials  grid (pixel chunks, images): per-pixel argmax, one ballot + popcount
//       per confusion cell, int32 counts per workgroup.
//   k_seg_conf_final  one workgroup: the partials summed by index in int64.
//   k_val_accumulate  one wave: val_loss = ((acc_steer + reverse) + seg) + depth in fp32, the
//       five values added to float64 running sums, the confusion matrix to an int64 running
//       matrix, the batch counter incremented; one packed buffer.
//   k_depth_metrics_partials  grid (cell chunks, images): per cell DepthLoss's class, the
//       argmax bin and the expected depth against the ground truth's metres (the reference
//       only draws these: trainer/pl_trainer.py:149-168); five counts and six float64 sums per
//       workgroup.
//   k_depth_metrics_final  one workgroup: each camera's records added by image, then chunk,
//       written out and added to the epoch's running buffer.
//   k_rollout_rows  one wave per row 3f + k of each sample: the free-running decoder's token
//       (ParkingModel.forward_rollout) against the ground-truth token and the teacher-forced
//       argmax (k_ctrl_val_rows' scan), detokenised against gt_acc / gt_steer / gt_reverse; one
//       record per row.
//   k_rollout_final  one workgroup: per future frame four float64 sums and eleven counts, the
//       samples added in index order, written out and added to the epoch's running buffer.
// One documented difference from the reference: it takes the argmax of the fp32 softmax, this
// file the argmax of the logits.  The two agree whenever the row's two largest logits are
// exactly equal (both pick the first index) and whenever they are far enough apart that their
// fp32 probabilities differ; between the two, distinct logits can round to equal
// probabilities, where the reference then picks the lower index and this kernel the larger
// logit.
// No atomics, nothing passed between workgroups inside a launch, every reduction in a fixed
// order, no host read: every launch is capturable.  A label value never forms an address: it
// is compared, or selects between two registers.
#include "argmax.h"
#include "common.h"

namespace e2ep {

constexpr int VAL_THREADS = 256;
constexpr int VAL_WAVES = VAL_THREADS / 64;
constexpr int CONF_MAX_C = 8;
constexpr int CONF_CELLS = CONF_MAX_C * CONF_MAX_C;  // cell slots per workgroup (C * C used)
constexpr int CONF_CHUNK = 2048;                     // pixels per workgroup, a multiple of 4

__device__ __forceinline__ float val_block_sum(float v, float *red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < VAL_WAVES; ++i) t += red[i];
  return t;
}

// torch SmoothL1Loss, beta = 1
__device__ __forceinline__ float smooth_l1(float x, float y) {
  const float d = fabsf(x - y);
  return d < 1.f ? 0.5f * d * d : d - 0.5f;
}

// the argmax token of one logits row in torch.argmax's order (argmax.h), by one wave: a strided
// scan per lane, then an xor butterfly, so every lane returns the row's token
__device__ __forceinline__ int row_argmax_token(const float *__restrict__ xr, int V, int lane) {
  float best = -INFINITY;
  int bi = 0x7fffffff;  // ranks below every real candidate of equal value
  for (int v = lane; v < V; v += 64) {
    const float a = xr[v];
    if (argmax_beats(a, v, best, bi)) best = a, bi = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (argmax_beats(ob, oi, best, bi)) best = ob, bi = oi;
  }
  return bi;
}

// detokenize_acc on a Python int: float64, rounded by np.float32 afterwards
template <typename I>
__device__ __forceinline__ float detok_acc(I tok, int valid_token) {
  const double half = (double)valid_token / 2.0, a = (double)tok / half - 1.0;
  return (float)((double)tok > half ? a : -a);
}

// detokenize_steer on an int64 tensor and a Python float: fp32 arithmetic
template <typename I>
__device__ __forceinline__ float detok_steer(I tok, int valid_token) {
  return (float)tok / (float)((double)valid_token / 2.0) - 1.f;
}

// row_vals: [acc | steer | reverse | reverse valid], B * F floats each
__global__ void __launch_bounds__(VAL_THREADS)
    k_ctrl_val_rows(const float *__restrict__ x, const float *__restrict__ gt_acc,
                    const float *__restrict__ gt_steer, const long long *__restrict__ gt_rev, int B,
                    int T, int V, int F, int valid_token, int split, int pad,
                    float *__restrict__ row_vals) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * VAL_WAVES + (threadIdx.x >> 6);
  const long long n = (long long)B * F;
  if (r >= n * 3) return;
  const int b = (int)(r / (3 * F)), j = (int)(r - (long long)b * 3 * F), f = j / 3, k = j - f * 3;
  const float *xr = x + ((long long)b * T + j) * V;
  const long long i = (long long)b * F + f;
  if (k < 2) {
    const int bi = row_argmax_token(xr, V, lane);
    if (lane == 0) {
      if (k == 0)
        row_vals[i] = smooth_l1(detok_acc(bi, valid_token), gt_acc[i]);
      else
        row_vals[n + i] = smooth_l1(detok_steer(bi, valid_token), gt_steer[i]);
    }
    return;
  }
  float m = -INFINITY;
  for (int v = lane; v < V; v += 64) m = fmaxf(m, xr[v]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float s = 0.f;
  for (int v = lane; v < V; v += 64) s += expf(xr[v] - m);
  s = wave_sum(s);
  float no = 0.f, yes = 0.f;
  for (int v = lane; v < V; v += 64) {
    const float p = expf(xr[v] - m) / s;
    no += v < split ? p : 0.f;
    yes += v < split ? 0.f : p;
  }
  no = wave_sum(no);
  yes = wave_sum(yes);
  if (lane == 0) {
    const long long t = gt_rev[i];
    const bool ok = t != pad && (t == 0 || t == 1);
    // cross entropy of the logits (no, yes): logsumexp - the target's
    const float mx = fmaxf(no, yes);
    const float lse = mx + logf(expf(no - mx) + expf(yes - mx));
    row_vals[2 * n + i] = ok ? lse - (t == 0 ? no : yes) : 0.f;
    row_vals[3 * n + i] = ok ? 1.f : 0.f;
  }
}

__global__ void __launch_bounds__(VAL_THREADS)
    k_ctrl_val_final(const float *__restrict__ row_vals, int n, float *__restrict__ out) {
  __shared__ float red[VAL_WAVES];
  float a = 0.f, s = 0.f, r = 0.f, c = 0.f;
  for (int i = threadIdx.x; i < n; i += VAL_THREADS) {
    a += row_vals[i];
    s += row_vals[(long long)n + i];
    r += row_vals[2LL * n + i];
    c += row_vals[3LL * n + i];
  }
  const float sa = val_block_sum(a, red), ss = val_block_sum(s, red);
  const float sr = val_block_sum(r, red), sc = val_block_sum(c, red);
  if (threadIdx.x == 0) {
    out[0] = sa / (float)n + ss / (float)n;
    out[1] = sc > 0.f ? sr / sc : NAN;  // torch: mean over zero rows is nan
  }
}

// ---- segmentation confusion matrix -----------------------------------------------------------
__device__ __forceinline__ int conf_class(const float (&v)[CONF_MAX_C], int C) {
  float best = v[0];
  int bi = 0;
#pragma unroll
  for (int k = 1; k < CONF_MAX_C; ++k)
    if (k < C && argmax_beats(v[k], k, best, bi)) {
      best = v[k];
      bi = k;
    }
  return bi;
}

// the wave's pixels of cell `cell` (-1: counted nowhere) added to the lane that owns the cell
__device__ __forceinline__ void conf_count(int cell, int cells, int lane, int &acc) {
  for (int c = 0; c < cells; ++c) {
    const int hits = __popcll(__ballot(cell == c));
    acc += lane == c ? hits : 0;
  }
}

// VEC: HW % 4 == 0 and logits 16-byte aligned: one float4 per plane per thread.  Otherwise
// dword loads.  Both paths visit the same pixels and add integers.
template <bool VEC>
__global__ void __launch_bounds__(VAL_THREADS)
    k_seg_conf_partials(const float *__restrict__ x, const long long *__restrict__ tg, int C, int HW,
                        int ignore, int *__restrict__ partials) {
  __shared__ int red[VAL_WAVES][CONF_CELLS];
  const int tid = threadIdx.x, lane = tid & 63, cells = C * C;
  const long long img = blockIdx.y;
  const int p0 = blockIdx.x * CONF_CHUNK, p1 = min(HW, p0 + CONF_CHUNK);
  const float *base = x + img * C * HW;
  const long long *tb = tg + img * HW;
  int acc = 0;
  // every wave runs the same number of iterations with all lanes active at the ballots
  if constexpr (VEC) {
    for (int q = p0 + tid * 4; q - tid * 4 < p1; q += VAL_THREADS * 4) {
      const bool in = q < p1;  // p1 - p0 is a multiple of 4 here
      float4 v[CONF_MAX_C];
#pragma unroll
      for (int k = 0; k < CONF_MAX_C; ++k)
        v[k] = in && k < C ? ld4(base + (long long)k * HW + q) : make_float4(0.f, 0.f, 0.f, 0.f);
      long long t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = in ? tb[q + j] : -1;
      float px[4][CONF_MAX_C];
#pragma unroll
      for (int k = 0; k < CONF_MAX_C; ++k) {
        px[0][k] = v[k].x;
        px[1][k] = v[k].y;
        px[2][k] = v[k].z;
        px[3][k] = v[k].w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = in && t[j] != ignore && t[j] >= 0 && t[j] < C;
        const int cell = ok ? (int)t[j] * C + conf_class(px[j], C) : -1;
        conf_count(cell, cells, lane, acc);
      }
    }
  } else {
    for (int q = p0 + tid; q - tid < p1; q += VAL_THREADS) {
      const bool in = q < p1;
      float v[CONF_MAX_C];
#pragma unroll
      for (int k = 0; k < CONF_MAX_C; ++k) v[k] = in && k < C ? base[(long long)k * HW + q] : 0.f;
      const long long t = in ? tb[q] : -1;
      const bool ok = in && t != ignore && t >= 0 && t < C;
      const int cell = ok ? (int)t * C + conf_class(v, C) : -1;
      conf_count(cell, cells, lane, acc);
    }
  }
  red[tid >> 6][lane] = acc;
  __syncthreads();
  if (tid < cells) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < VAL_WAVES; ++w) s += red[w][tid];
    partials[(img * gridDim.x + blockIdx.x) * CONF_CELLS + tid] = s;
  }
}

// one workgroup: thread (slice, cell) sums every VAL_WAVES-th workgroup's count of its cell,
// then the slices are added in order
__global__ void __launch_bounds__(VAL_THREADS)
    k_seg_conf_final(const int *__restrict__ partials, int nblocks, int cells,
                     long long *__restrict__ conf) {
  __shared__ long long red[VAL_WAVES][CONF_CELLS];
  const int cell = threadIdx.x & 63, slice = threadIdx.x >> 6;
  long long s = 0;
  if (cell < cells)
    for (int i = slice; i < nblocks; i += VAL_WAVES) s += partials[(long long)i * CONF_CELLS + cell];
  red[slice][cell] = s;
  __syncthreads();
  if (threadIdx.x < cells) {
    long long t = 0;
#pragma unroll
    for (int w = 0; w < VAL_WAVES; ++w) t += red[w][threadIdx.x];
    conf[threadIdx.x] = t;
  }
}

// ---- epoch accumulator ------------------------------------------------------------------------
// packed: double sums[5] (acc_steer, reverse, segmentation, depth, val_loss) | int64 batches |
// int64 conf[cells]
__global__ void __launch_bounds__(64)
    k_val_accumulate(const float *__restrict__ control, const float *__restrict__ seg,
                     const float *__restrict__ depth, const long long *__restrict__ conf, int cells,
                     double *__restrict__ sums, long long *__restrict__ counts,
                     float *__restrict__ val_loss) {
  const int lane = threadIdx.x;
  if (lane < cells) counts[1 + lane] += conf[lane];
  if (lane == 0) {
    const float a = control[0], r = control[1], s = seg[0], d = depth[0];
    const float v = ((a + r) + s) + d;  // Python's sum(d.values())
    val_loss[0] = v;
    sums[0] += (double)a;
    sums[1] += (double)r;
    sums[2] += (double)s;
    sums[3] += (double)d;
    sums[4] += (double)v;
    counts[0] += 1;
  }
}

inline int conf_chunks(int HW) { return cdiv(HW, CONF_CHUNK); }

// ---- depth-head metrics -----------------------------------------------------------------------
// One thread per cell (a down x down block of gt), one workgroup per DM_CHUNK cells of one image,
// so a workgroup belongs to one camera (bn % N).  A partial record is DM_SUMS doubles followed
// by DM_COUNTS int64, in the order of e2ep.h; k_depth_metrics_final adds each camera's records
// by image, then chunk.
constexpr int DM_CHUNK = VAL_THREADS;  // cells per workgroup
constexpr int DM_SUMS = 6, DM_COUNTS = 5, DM_REC = DM_SUMS + DM_COUNTS;
constexpr int DM_MAX_CAMS = 16;
static_assert(DM_MAX_CAMS * DM_REC <= VAL_THREADS, "k_depth_metrics_final: one thread per entry");

template <typename T, int V> using dm_vec = T __attribute__((ext_vector_type(V)));

// the block's value of thread v in lane 0 of wave 0: xor butterflies, then the waves in order
template <typename A>
__device__ __forceinline__ A dm_block_sum(A v, A *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  A t = red[0];
#pragma unroll
  for (int i = 1; i < VAL_WAVES; ++i) t += red[i];
  return t;
}

// T: the ground truth's type, as k_depth_bce_fwd<T> (loss.hip), whose class statement this
// repeats.  VEC: 16-byte loads of gt (down, W multiples of 16 / sizeof(T) elements and gt
// 16-byte aligned), otherwise element loads; the min does not depend on the order.
template <typename T, bool VEC>
__global__ void __launch_bounds__(VAL_THREADS)
    k_depth_metrics_partials(const float *__restrict__ prob, const T *__restrict__ gt, int D, int H,
                             int W, int down, T lo, T step, double d0, double dstep,
                             float *__restrict__ pred_map, float *__restrict__ gt_map,
                             int *__restrict__ cls_out, double *__restrict__ partials) {
  __shared__ double red_d[VAL_WAVES];
  __shared__ long long red_i[VAL_WAVES];
  constexpr int V = 16 / (int)sizeof(T);
  const int h = H / down, w = W / down, hw = h * w;
  const long long bn = blockIdx.y;
  const int pix = blockIdx.x * DM_CHUNK + threadIdx.x;
  double s[DM_SUMS] = {0., 0., 0., 0., 0., 0.};
  long long n[DM_COUNTS] = {0, 0, 0, 0, 0};
  if (pix < hw) {
    const int ci = pix / w, cj = pix - ci * w;
    const T *g = gt + (bn * H + (long long)ci * down) * W + (long long)cj * down;
    T mn = T(1e5);
    for (int r = 0; r < down; ++r) {
      if constexpr (VEC) {
        for (int c = 0; c < down; c += V) {
          const dm_vec<T, V> d = *reinterpret_cast<const dm_vec<T, V> *>(g + (long long)r * W + c);
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const T e = d[j] == T(0) ? T(1e5) : d[j];
            mn = e < mn ? e : mn;
          }
        }
      } else {
        for (int c = 0; c < down; ++c) {
          const T d = g[(long long)r * W + c];
          const T e = d == T(0) ? T(1e5) : d;
          mn = e < mn ? e : mn;
        }
      }
    }
    const T b = (mn - lo) / step;
    const int k = (b < T(D + 1) && b >= T(0)) ? (int)b : 0;
    const long long cell = bn * hw + pix;
    if (cls_out) cls_out[cell] = k;
    if (gt_map) gt_map[cell] = k >= 1 ? (float)mn : 0.f;
    if (k >= 1 || pred_map) {
      const float *pp = prob + bn * D * hw + pix;
      const int t = k - 1;
      float best = pp[0], pt = best;
      int a = 0;
      double ze = (double)best * d0;
      for (int d = 1; d < D; ++d) {
        const float p = pp[(long long)d * hw];
        if (argmax_beats(p, d, best, a)) best = p, a = d;
        pt = d == t ? p : pt;
        ze += (double)p * (d0 + (double)d * dstep);
      }
      const double za = d0 + (double)a * dstep;
      if (pred_map) pred_map[cell] = (float)za;
      if (k >= 1) {
        const double gm = (double)mn, ea = fabs(za - gm), ee = fabs(ze - gm);
        const int db = a > t ? a - t : t - a;
        n[0] = 1;
        n[1] = db == 0;
        n[2] = db <= 1;
        n[3] = db;
        n[4] = za < 1.25 * gm && gm < 1.25 * za;
        s[0] = ea;
        s[1] = (za - gm) * (za - gm);
        s[2] = ea / gm;
        s[3] = ee;
        s[4] = (ze - gm) * (ze - gm);
        s[5] = (double)pt;
      }
    }
  }
  double *rec = partials + (bn * gridDim.x + blockIdx.x) * DM_REC;
#pragma unroll
  for (int e = 0; e < DM_SUMS; ++e) {
    const double v = dm_block_sum(s[e], red_d);
    if (threadIdx.x == 0) rec[e] = v;
  }
#pragma unroll
  for (int e = 0; e < DM_COUNTS; ++e) {
    const long long v = dm_block_sum(n[e], red_i);
    if (threadIdx.x == 0) reinterpret_cast<long long *>(rec)[DM_SUMS + e] = v;
  }
}

// one workgroup: thread (camera, entry) adds the camera's records image by image, chunk by
// chunk, writes out and adds it to running.  out / running: double sums[N][6] | int64
// counts[N][5] (| int64 batches)
__global__ void __launch_bounds__(VAL_THREADS)
    k_depth_metrics_final(const double *__restrict__ partials, int BN, int N, int chunks,
                          double *__restrict__ out, double *__restrict__ running) {
  const int cam = threadIdx.x / DM_REC, e = threadIdx.x - cam * DM_REC;
  if (cam < N) {
    if (e < DM_SUMS) {
      double v = 0.;
      for (int bn = cam; bn < BN; bn += N)
        for (int c = 0; c < chunks; ++c) v += partials[((long long)bn * chunks + c) * DM_REC + e];
      out[cam * DM_SUMS + e] = v;
      if (running) running[cam * DM_SUMS + e] += v;
    } else {
      const long long *pi = reinterpret_cast<const long long *>(partials);
      const int slot = N * DM_SUMS + cam * DM_COUNTS + (e - DM_SUMS);
      long long v = 0;
      for (int bn = cam; bn < BN; bn += N)
        for (int c = 0; c < chunks; ++c) v += pi[((long long)bn * chunks + c) * DM_REC + e];
      reinterpret_cast<long long *>(out)[slot] = v;
      if (running) reinterpret_cast<long long *>(running)[slot] += v;
    }
  }
  if (threadIdx.x == 0 && running) reinterpret_cast<long long *>(running)[N * DM_REC] += 1;
}

inline bool dm_shape_ok(int BN, int N, int H, int W, int down) {
  return N >= 1 && N <= DM_MAX_CAMS && BN > 0 && BN % N == 0 && down > 0 && H > 0 && W > 0 &&
         H % down == 0 && W % down == 0;
}
inline int dm_chunks(int H, int W, int down) {
  return cdiv((long long)(H / down) * (W / down), DM_CHUNK);
}

// ---- free-running rollout metrics -----------------------------------------------------------
// Row (b, j), j = 3f + k, compares the decoder's own token p = seq[b][1 + j] with the ground
// truth g = gt_control[b][1 + j] and the teacher-forced argmax a of logits[b][j].  Its record
// in the workspace is three 8-byte words: two float64 terms and an int64 of flag bits.
//   k = 0  |acc_s - gt_acc|, smooth_l1(acc_v, gt_acc): acc_s the signed acceleration, acc_v
//          detokenize_acc's folded one (detok_acc)
//   k = 1  |steer - gt_steer|, smooth_l1(steer, gt_steer)
//   k = 2  0, 0
// Each term in float64 from two fp32 values.  A token is compared or converted to a number; it
// never forms an address.
constexpr int RO_SUMS = 4, RO_COUNTS = 11, RO_REC = RO_SUMS + RO_COUNTS, RO_WORDS = 3;
constexpr long long RO_HIT = 1, RO_AGREE = 2, RO_INVALID = 4, RO_REVERSE = 8;

__device__ __forceinline__ double smooth_l1_f64(float x, float y) {
  const double d = fabs((double)x - (double)y);
  return d < 1.0 ? 0.5 * d * d : d - 0.5;
}

__global__ void __launch_bounds__(VAL_THREADS)
    k_rollout_rows(const long long *__restrict__ seq, long long seq_stride,
                   const float *__restrict__ logits, const long long *__restrict__ gt_control,
                   const float *__restrict__ gt_acc, const float *__restrict__ gt_steer,
                   const long long *__restrict__ gt_rev, int B, int F, int V, int valid_token,
                   double *__restrict__ recs) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * VAL_WAVES + (threadIdx.x >> 6);
  const int J = 3 * F, T = J + 2;
  if (r >= (long long)B * J) return;
  const int b = (int)(r / J), j = (int)(r - (long long)b * J), f = j / 3, k = j - f * 3;
  const int a = logits ? row_argmax_token(logits + ((long long)b * T + j) * V, V, lane) : -1;
  if (lane != 0) return;
  const long long p = seq[(long long)b * seq_stride + 1 + j];
  const long long g = gt_control[(long long)b * (T + 1) + 1 + j];
  const long long i = (long long)b * F + f;
  long long flags = (p == g ? RO_HIT : 0) | (logits && p == (long long)a ? RO_AGREE : 0) |
                    (p > (long long)valid_token ? RO_INVALID : 0);
  double v0 = 0., v1 = 0.;
  const double half = (double)valid_token / 2.0;
  if (k == 0) {
    const float y = gt_acc[i], acc_s = (float)((double)p / half - 1.0);
    v0 = fabs((double)acc_s - (double)y);
    v1 = smooth_l1_f64(detok_acc(p, valid_token), y);
  } else if (k == 1) {
    const float y = gt_steer[i], steer = detok_steer(p, valid_token);
    v0 = fabs((double)steer - (double)y);
    v1 = smooth_l1_f64(steer, y);
  } else {
    const long long t = gt_rev[i];
    const bool rev = (double)p > half;  // detokenize's rule
    flags |= (t == 1 ? rev : (t == 0 && !rev)) ? RO_REVERSE : 0;
  }
  double *rec = recs + r * RO_WORDS;
  rec[0] = v0;
  rec[1] = v1;
  reinterpret_cast<long long *>(rec)[2] = flags;
}

// one workgroup: thread (frame, entry) adds its quantity over the samples in index order,
// writes out and adds it to running.  out / running: double sums[F][4] | int64 counts[F][11]
// (| int64 batches)
__global__ void __launch_bounds__(VAL_THREADS)
    k_rollout_final(const double *__restrict__ recs, int B, int F, double *__restrict__ out,
                    double *__restrict__ running) {
  const int J = 3 * F;
  const long long *words = reinterpret_cast<const long long *>(recs);
  for (int idx = threadIdx.x; idx < F * RO_REC; idx += VAL_THREADS) {
    const int f = idx / RO_REC, e = idx - f * RO_REC;
    if (e < RO_SUMS) {
      // e = 0, 1: the first term of rows k = 0, 1; e = 2, 3: the second
      const int k = e & 1, w = e >> 1;
      double v = 0.;
      for (int b = 0; b < B; ++b) v += recs[((long long)b * J + 3 * f + k) * RO_WORDS + w];
      out[f * RO_SUMS + e] = v;
      if (running) running[f * RO_SUMS + e] += v;
    } else {
      const int c = e - RO_SUMS;
      long long v = 0;
      for (int b = 0; b < B; ++b) {
        const long long *row = words + ((long long)b * J + 3 * f) * RO_WORDS + 2;
        const long long f0 = row[0], f1 = row[RO_WORDS], f2 = row[2 * RO_WORDS];
        long long hit;
        if (c == 0) {
          hit = 1;
        } else if (c <= 3) {
          hit = ((c == 1 ? f0 : c == 2 ? f1 : f2) & RO_HIT) != 0;
        } else if (c == 4) {
          hit = (f0 & f1 & f2 & RO_HIT) != 0;
        } else if (c == 5) {
          long long all = RO_HIT;
          for (int j = 0; j < 3 * f + 3; ++j) all &= words[((long long)b * J + j) * RO_WORDS + 2];
          hit = all != 0;
        } else if (c == 6) {
          hit = (f2 & RO_REVERSE) != 0;
        } else if (c == 7) {
          hit = ((f0 | f1 | f2) & RO_INVALID) != 0;
        } else {
          hit = ((c == 8 ? f0 : c == 9 ? f1 : f2) & RO_AGREE) != 0;
        }
        v += hit;
      }
      const int slot = F * RO_SUMS + f * RO_COUNTS + c;
      reinterpret_cast<long long *>(out)[slot] = v;
      if (running) reinterpret_cast<long long *>(running)[slot] += v;
    }
  }
  if (threadIdx.x == 0 && running) reinterpret_cast<long long *>(running)[F * RO_REC] += 1;
}

}  // namespace e2ep

using namespace e2ep;

template <typename T>
static int depth_metrics(const char *name, const float *prob, const T *gt, int BN, int N, int D,
                         int H, int W, int down, T lo, T step, double d0, double dstep, void *out,
                         void *running, float *pred_map, float *gt_map, int *cls_out,
                         void *workspace, size_t workspace_bytes, void *stream) {
  E2EP_REQUIRE(prob && gt && out && workspace, E2EP_EINVAL, "%s: null argument", name);
  E2EP_REQUIRE(dm_shape_ok(BN, N, H, W, down) && D > 0, E2EP_EINVAL,
               "%s: bad shape (BN=%d N=%d (1..%d, dividing BN) D=%d H=%d W=%d down=%d)", name, BN,
               N, DM_MAX_CAMS, D, H, W, down);
  E2EP_REQUIRE(BN <= 65535 && (long long)(H / down) * (W / down) <= 0x7fff0000LL, E2EP_ERANGE,
               "%s: BN=%d images of %d x %d cells exceed the grid", name, BN, H / down, W / down);
  E2EP_REQUIRE(workspace_bytes >= e2ep_depth_metrics_workspace(BN, N, H, W, down), E2EP_EINVAL,
               "%s: workspace %zu < %zu bytes", name, workspace_bytes,
               e2ep_depth_metrics_workspace(BN, N, H, W, down));
  E2EP_REQUIRE(((uintptr_t)prob & 3) == 0 && (uintptr_t)gt % sizeof(T) == 0 &&
                   ((uintptr_t)out & 7) == 0 && ((uintptr_t)running & 7) == 0 &&
                   ((uintptr_t)pred_map & 3) == 0 && ((uintptr_t)gt_map & 3) == 0 &&
                   ((uintptr_t)cls_out & 3) == 0 && ((uintptr_t)workspace & 7) == 0,
               E2EP_EINVAL, "%s: misaligned buffer", name);
  constexpr int V = 16 / (int)sizeof(T);
  const int chunks = dm_chunks(H, W, down);
  const dim3 grid(chunks, BN), block(VAL_THREADS);
  double *part = static_cast<double *>(workspace);
  if (down % V == 0 && W % V == 0 && ((uintptr_t)gt & 15) == 0)
    hipLaunchKernelGGL((k_depth_metrics_partials<T, true>), grid, block, 0, as_stream(stream), prob,
                       gt, D, H, W, down, lo, step, d0, dstep, pred_map, gt_map, cls_out, part);
  else
    hipLaunchKernelGGL((k_depth_metrics_partials<T, false>), grid, block, 0, as_stream(stream),
                       prob, gt, D, H, W, down, lo, step, d0, dstep, pred_map, gt_map, cls_out,
                       part);
  hipLaunchKernelGGL(k_depth_metrics_final, dim3(1), dim3(VAL_THREADS), 0, as_stream(stream), part,
                     BN, N, chunks, static_cast<double *>(out), static_cast<double *>(running));
  return launch_status(name);
}

extern "C" {

size_t e2ep_depth_metrics_workspace(int BN, int N, int H, int W, int down) {
  if (!dm_shape_ok(BN, N, H, W, down)) return 0;
  return (size_t)BN * dm_chunks(H, W, down) * DM_REC * sizeof(double);
}

int e2ep_depth_metrics(const float *prob, const float *gt, int BN, int N, int D, int H, int W,
                       int down, float lo, float step, double d0, double dstep, void *out,
                       void *running, float *pred_map, float *gt_map, int *cls_out,
                       void *workspace, size_t workspace_bytes, void *stream) {
  return depth_metrics("e2ep_depth_metrics", prob, gt, BN, N, D, H, W, down, lo, step, d0, dstep,
                       out, running, pred_map, gt_map, cls_out, workspace, workspace_bytes, stream);
}

int e2ep_depth_metrics_f64(const float *prob, const double *gt, int BN, int N, int D, int H, int W,
                           int down, double lo, double step, double d0, double dstep, void *out,
                           void *running, float *pred_map, float *gt_map, int *cls_out,
                           void *workspace, size_t workspace_bytes, void *stream) {
  return depth_metrics("e2ep_depth_metrics_f64", prob, gt, BN, N, D, H, W, down, lo, step, d0,
                       dstep, out, running, pred_map, gt_map, cls_out, workspace, workspace_bytes,
                       stream);
}

size_t e2ep_control_val_workspace(int B, int F) {
  if (B <= 0 || F <= 0) return 0;
  return (size_t)B * F * 4 * sizeof(float);
}

int e2ep_control_val_fwd(const float *logits, const float *gt_acc, const float *gt_steer,
                         const long long *gt_reverse, int B, int T, int vocab, int F,
                         int valid_token, int split, int pad, float *out, void *workspace,
                         size_t workspace_bytes, void *stream) {
  E2EP_REQUIRE(logits && gt_acc && gt_steer && gt_reverse && out && workspace, E2EP_EINVAL,
               "e2ep_control_val_fwd: null argument");
  E2EP_REQUIRE(B > 0 && T >= 5 && (T - 2) % 3 == 0 && F == (T - 2) / 3, E2EP_EINVAL,
               "e2ep_control_val_fwd: T=%d must be 3 F + 2 with F=%d labels per sample (B=%d)", T,
               F, B);
  E2EP_REQUIRE(vocab > 0 && valid_token > 0 && split >= 0 && split <= vocab, E2EP_EINVAL,
               "e2ep_control_val_fwd: bad vocabulary (vocab=%d valid_token=%d split=%d)", vocab,
               valid_token, split);
  E2EP_REQUIRE((long long)B * F * 3 <= 0x7fffffffLL / 4, E2EP_ERANGE,
               "e2ep_control_val_fwd: B * F = %lld rows exceed the grid", (long long)B * F);
  E2EP_REQUIRE(workspace_bytes >= e2ep_control_val_workspace(B, F), E2EP_EINVAL,
               "e2ep_control_val_fwd: workspace %zu < %zu bytes", workspace_bytes,
               e2ep_control_val_workspace(B, F));
  E2EP_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)gt_acc & 3) == 0 &&
                   ((uintptr_t)gt_steer & 3) == 0 && ((uintptr_t)gt_reverse & 7) == 0 &&
                   ((uintptr_t)out & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
               E2EP_EINVAL, "e2ep_control_val_fwd: misaligned buffer");
  const int n = B * F;
  float *row_vals = static_cast<float *>(workspace);
  hipLaunchKernelGGL(k_ctrl_val_rows, dim3(cdiv((long long)n * 3, VAL_WAVES)), dim3(VAL_THREADS), 0,
                     as_stream(stream), logits, gt_acc, gt_steer, gt_reverse, B, T, vocab, F,
                     valid_token, split, pad, row_vals);
  hipLaunchKernelGGL(k_ctrl_val_final, dim3(1), dim3(VAL_THREADS), 0, as_stream(stream), row_vals,
                     n, out);
  return launch_status("e2ep_control_val_fwd");
}

size_t e2ep_rollout_metrics_workspace(int B, int F) {
  if (B <= 0 || F <= 0) return 0;
  return (size_t)B * 3 * F * RO_WORDS * sizeof(double);
}

int e2ep_rollout_metrics(const long long *seq, long long seq_stride, const float *logits,
                         const long long *gt_control, const float *gt_acc, const float *gt_steer,
                         const long long *gt_reverse, int B, int F, int vocab, int valid_token,
                         void *out, void *running, void *workspace, size_t workspace_bytes,
                         void *stream) {
  E2EP_REQUIRE(seq && gt_control && gt_acc && gt_steer && gt_reverse && out && workspace,
               E2EP_EINVAL, "e2ep_rollout_metrics: null argument");
  E2EP_REQUIRE(B >= 1 && F >= 1, E2EP_EINVAL, "e2ep_rollout_metrics: bad shape (B=%d F=%d)", B, F);
  E2EP_REQUIRE(vocab >= 5 && valid_token >= 1, E2EP_EINVAL,
               "e2ep_rollout_metrics: bad vocabulary (vocab=%d, at least 5; valid_token=%d)", vocab,
               valid_token);
  E2EP_REQUIRE((long long)B * F * 3 <= 0x7fffffffLL / 4, E2EP_ERANGE,
               "e2ep_rollout_metrics: B * F = %lld rows exceed the grid", (long long)B * F);
  E2EP_REQUIRE(seq_stride >= 1 + 3LL * F, E2EP_EINVAL,
               "e2ep_rollout_metrics: seq row stride %lld < 1 + 3 F = %lld", seq_stride,
               1 + 3LL * F);
  E2EP_REQUIRE(workspace_bytes >= e2ep_rollout_metrics_workspace(B, F), E2EP_EINVAL,
               "e2ep_rollout_metrics: workspace %zu < %zu bytes", workspace_bytes,
               e2ep_rollout_metrics_workspace(B, F));
  E2EP_REQUIRE(((uintptr_t)seq & 7) == 0 && ((uintptr_t)logits & 3) == 0 &&
                   ((uintptr_t)gt_control & 7) == 0 && ((uintptr_t)gt_acc & 3) == 0 &&
                   ((uintptr_t)gt_steer & 3) == 0 && ((uintptr_t)gt_reverse & 7) == 0 &&
                   ((uintptr_t)out & 7) == 0 && ((uintptr_t)running & 7) == 0 &&
                   ((uintptr_t)workspace & 7) == 0,
               E2EP_EINVAL, "e2ep_rollout_metrics: misaligned buffer");
  double *recs = static_cast<double *>(workspace);
  hipLaunchKernelGGL(k_rollout_rows, dim3(cdiv((long long)B * F * 3, VAL_WAVES)),
                     dim3(VAL_THREADS), 0, as_stream(stream), seq, seq_stride, logits, gt_control,
                     gt_acc, gt_steer, gt_reverse, B, F, vocab, valid_token, recs);
  hipLaunchKernelGGL(k_rollout_final, dim3(1), dim3(VAL_THREADS), 0, as_stream(stream), recs, B, F,
                     static_cast<double *>(out), static_cast<double *>(running));
  return launch_status("e2ep_rollout_metrics");
}

size_t e2ep_seg_confusion_workspace(int images, int HW) {
  if (images <= 0 || HW <= 0) return 0;
  return (size_t)images * conf_chunks(HW) * CONF_CELLS * sizeof(int);
}

int e2ep_seg_confusion(const float *logits, const long long *target, int images, int C, int HW,
                       int ignore, int64_t *conf, void *workspace, size_t workspace_bytes,
                       void *stream) {
  E2EP_REQUIRE(logits && target && conf && workspace, E2EP_EINVAL,
               "e2ep_seg_confusion: null argument");
  E2EP_REQUIRE(C >= 2 && C <= CONF_MAX_C, E2EP_EINVAL, "e2ep_seg_confusion: C=%d outside 2..%d", C,
               CONF_MAX_C);
  E2EP_REQUIRE(images > 0 && HW > 0, E2EP_EINVAL, "e2ep_seg_confusion: bad shape (images=%d HW=%d)",
               images, HW);
  E2EP_REQUIRE(images <= 65535 && HW <= 0x7fff0000 &&
                   (long long)images * conf_chunks(HW) <= 0x7fffffffLL / CONF_CELLS,
               E2EP_ERANGE, "e2ep_seg_confusion: images=%d HW=%d exceed the grid", images, HW);
  E2EP_REQUIRE(workspace_bytes >= e2ep_seg_confusion_workspace(images, HW), E2EP_EINVAL,
               "e2ep_seg_confusion: workspace %zu < %zu bytes", workspace_bytes,
               e2ep_seg_confusion_workspace(images, HW));
  E2EP_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)target & 7) == 0 &&
                   ((uintptr_t)conf & 7) == 0 && ((uintptr_t)workspace & 3) == 0,
               E2EP_EINVAL, "e2ep_seg_confusion: misaligned buffer");
  const int chunks = conf_chunks(HW);
  const dim3 grid(chunks, images), block(VAL_THREADS);
  int *part = static_cast<int *>(workspace);
  if (HW % 4 == 0 && ((uintptr_t)logits & 15) == 0)
    hipLaunchKernelGGL(k_seg_conf_partials<true>, grid, block, 0, as_stream(stream), logits, target,
                       C, HW, ignore, part);
  else
    hipLaunchKernelGGL(k_seg_conf_partials<false>, grid, block, 0, as_stream(stream), logits,
                       target, C, HW, ignore, part);
  hipLaunchKernelGGL(k_seg_conf_final, dim3(1), dim3(VAL_THREADS), 0, as_stream(stream), part,
                     images * chunks, C * C, reinterpret_cast<long long *>(conf));
  return launch_status("e2ep_seg_confusion");
}

int e2ep_val_accumulate(const float *control, const float *seg, const float *depth,
                        const int64_t *conf, int C, void *packed, float *val_loss, void *stream) {
  E2EP_REQUIRE(control && seg && depth && packed && val_loss, E2EP_EINVAL,
               "e2ep_val_accumulate: null argument");
  E2EP_REQUIRE(conf ? (C >= 2 && C <= CONF_MAX_C) : C == 0, E2EP_EINVAL,
               "e2ep_val_accumulate: C=%d (2..%d with a confusion matrix, 0 without)", C,
               CONF_MAX_C);
  E2EP_REQUIRE(((uintptr_t)control & 3) == 0 && ((uintptr_t)seg & 3) == 0 &&
                   ((uintptr_t)depth & 3) == 0 && ((uintptr_t)conf & 7) == 0 &&
                   ((uintptr_t)packed & 7) == 0 && ((uintptr_t)val_loss & 3) == 0,
               E2EP_EINVAL, "e2ep_val_accumulate: misaligned buffer");
  double *sums = static_cast<double *>(packed);
  hipLaunchKernelGGL(k_val_accumulate, dim3(1), dim3(64), 0, as_stream(stream), control, seg, depth,
                     reinterpret_cast<const long long *>(conf), C * C, sums,
                     reinterpret_cast<long long *>(sums + 5), val_loss);
  return launch_status("e2ep_val_accumulate");
}

}  // extern "C"
