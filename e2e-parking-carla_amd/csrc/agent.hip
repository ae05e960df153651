// The closed-loop agent's per-frame post-processing, on the GPU.
//
// After every ParkingModel.predict the reference agent (agent/parking_agent.py) runs on the
// host:
//   save_prev_target (:290-311)  torch.argmax over the (3, 200, 200) segmentation logits, a
//       synchronising .cpu(), the image flipped top to bottom ([::-1]), a Python double loop
//       over all 40 000 pixels collecting the coordinates of class 2 (the target slot),
//       int(np.average(...)) per axis;
//   get_target_point_ego_coord (:313-318)  pixel -> ego frame, both axes offset by
//       shape[0] / 2, times the BEV resolution; the result replaces target_point[:2] of the
//       next frame (get_model_data :474-476), the yaw still coming from the goal;
//   save_seg_img (:272-281)  with the display on, the same argmax again for the 0 / 128 / 255
//       class image;
//   detokenize (dataset/carla_dataset.py:90-111) of the three predicted control tokens.
// Everything is integer counts and sums, one integer division and one float64 multiply, so
// the kernels below reproduce it bit for bit:
//   k_slot_partials  grid (row bands, B): per-pixel class by torch.argmax's order
//       (argmax.h), integer partials (count, sum of flipped rows, sum of columns) of the
//       target class per workgroup, optionally the flipped class image through a lookup
//       table.  No atomics, no communication between workgroups.
//   k_slot_finish    one wave per sample: the partials summed in int64, the two integer
//       means, the ego-frame point into the persistent per-sample state (left untouched when
//       no pixel has the class), plus the detokenized controls of that sample's token row.
//   k_target_select  target_used[b] = state valid ? (px, py, goal yaw) : goal.
// The maps are small (480 KB of logits per sample at the agent's shape), so the kernels are
// latency-bound: a band is a few rows, which spreads one sample over a few dozen workgroups,
// and each thread has all C plane loads of its pixels in flight before it compares.
#include "argmax.h"
#include "common.h"

namespace e2ep {

constexpr int AG_THREADS = 256;
constexpr int AG_MAX_C = 8;
constexpr int AG_BANDS = 48;  // row bands aimed at per sample

inline int slot_band_rows(int X) { return cdiv(X, AG_BANDS); }
inline int slot_bands(int X) { return cdiv(X, slot_band_rows(X)); }

struct SlotArgs {
  int C, X, Y, rows;          // rows per band
  long long sb, sc, sx, sy;   // element strides of logits (B, C, X, Y)
  int target;                 // the class whose pixels are counted
  unsigned long long lut;     // class image value of class k in byte k
};

// (count, sum of flipped row, sum of column) of the target-class pixels of one thread
struct SlotAcc {
  int n, sr, sc;
  __device__ __forceinline__ void add(bool hit, int fr, int c) {
    n += hit ? 1 : 0;
    sr += hit ? fr : 0;
    sc += hit ? c : 0;
  }
};

// class of one pixel from its C logits (v[k] valid for k < C): torch.argmax's order
__device__ __forceinline__ int pixel_class(const float (&v)[AG_MAX_C], int C) {
  float best = v[0];
  int bi = 0;
#pragma unroll
  for (int k = 1; k < AG_MAX_C; ++k)
    if (k < C && argmax_beats(v[k], k, best, bi)) {
      best = v[k];
      bi = k;
    }
  return bi;
}

// VEC: sy == 1, Y % 4 == 0 and every plane row 16-byte aligned: one float4 per plane per
// thread, four class-image bytes as one dword store.  Otherwise dword loads through the
// element strides and byte stores.  Both paths visit the same pixels and add integers.
template <bool VEC>
__global__ void __launch_bounds__(AG_THREADS)
    k_slot_partials(const float *__restrict__ logits, SlotArgs a, int *__restrict__ partials,
                    unsigned char *__restrict__ cls_img) {
  __shared__ int red[AG_THREADS / 64][3];
  const int band = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int r0 = band * a.rows, r1 = min(a.X, r0 + a.rows);
  const float *base = logits + (long long)b * a.sb;
  unsigned char *img = cls_img ? cls_img + (long long)b * a.X * a.Y : nullptr;
  SlotAcc acc = {0, 0, 0};
  if constexpr (VEC) {
    const int yq = a.Y / 4, nq = (r1 - r0) * yq;
    for (int q = tid; q < nq; q += AG_THREADS) {
      const int r = r0 + q / yq, c = (q % yq) * 4, fr = a.X - 1 - r;
      const float *p = base + (long long)r * a.sx + c;
      float4 v[AG_MAX_C];
#pragma unroll
      for (int k = 0; k < AG_MAX_C; ++k)
        v[k] = k < a.C ? ld4(p + (long long)k * a.sc) : make_float4(0.f, 0.f, 0.f, 0.f);
      float px[4][AG_MAX_C];
#pragma unroll
      for (int k = 0; k < AG_MAX_C; ++k) {
        px[0][k] = v[k].x;
        px[1][k] = v[k].y;
        px[2][k] = v[k].z;
        px[3][k] = v[k].w;
      }
      unsigned packed = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cls = pixel_class(px[j], a.C);
        acc.add(cls == a.target, fr, c + j);
        packed |= (unsigned)((a.lut >> (8 * cls)) & 0xffu) << (8 * j);
      }
      if (img) *reinterpret_cast<unsigned *>(img + (long long)fr * a.Y + c) = packed;
    }
  } else {
    const int np = (r1 - r0) * a.Y;
    for (int i = tid; i < np; i += AG_THREADS) {
      const int r = r0 + i / a.Y, c = i % a.Y, fr = a.X - 1 - r;
      const float *p = base + (long long)r * a.sx + (long long)c * a.sy;
      float v[AG_MAX_C];
#pragma unroll
      for (int k = 0; k < AG_MAX_C; ++k)
        v[k] = k < a.C ? p[(long long)k * a.sc] : 0.f;
      const int cls = pixel_class(v, a.C);
      acc.add(cls == a.target, fr, c);
      if (img) img[(long long)fr * a.Y + c] = (unsigned char)((a.lut >> (8 * cls)) & 0xffu);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc.n += __shfl_xor(acc.n, o, 64);
    acc.sr += __shfl_xor(acc.sr, o, 64);
    acc.sc += __shfl_xor(acc.sc, o, 64);
  }
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = acc.n;
    red[tid >> 6][1] = acc.sr;
    red[tid >> 6][2] = acc.sc;
  }
  __syncthreads();
  if (tid < 3) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < AG_THREADS / 64; ++w) s += red[w][tid];
    partials[((long long)b * gridDim.x + band) * 3 + tid] = s;
  }
}

struct FinishArgs {
  int bands, X;
  double res_x, res_y;
  const long long *seq;  // token rows (may be null: no detokenize)
  int seq_stride, seq_len, first, token_nums;
};

// grid B, one wave
__global__ void __launch_bounds__(64)
    k_slot_finish(const int *__restrict__ partials, FinishArgs a, float *__restrict__ state,
                  int *__restrict__ found, long long *__restrict__ stats,
                  double *__restrict__ controls, long long *__restrict__ tokens_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  long long n = 0, sr = 0, sc = 0;
  for (int i = lane; i < a.bands; i += 64) {
    const int *p = partials + ((long long)b * a.bands + i) * 3;
    n += p[0];
    sr += p[1];
    sc += p[2];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_xor(n, o, 64);
    sr += __shfl_xor(sr, o, 64);
    sc += __shfl_xor(sc, o, 64);
  }
  if (lane == 0) {
    long long tx = -1, ty = -1;
    if (n > 0) {
      // int(np.average(...)): the values are non-negative, so truncation is integer division
      tx = sr / n;
      ty = sc / n;
      // get_target_point_ego_coord: shape[0] / 2 on both axes, float64, then the fp32 tensor
      const double half = a.X / 2.0;
      const double x = -((double)tx - half), y = (double)ty - half;
      state[b * 3 + 0] = 1.f;
      state[b * 3 + 1] = (float)(x * a.res_x);
      state[b * 3 + 2] = (float)(y * a.res_y);
    }
    if (found) found[b] = n > 0 ? 1 : 0;
    if (stats) {
      stats[b * 3 + 0] = n;
      stats[b * 3 + 1] = tx;
      stats[b * 3 + 2] = ty;
    }
  }
  if (!a.seq) return;
  const long long *row = a.seq + (long long)b * a.seq_stride;
  if (tokens_out)
    for (int t = lane; t < a.seq_len; t += 64) tokens_out[(long long)b * a.seq_len + t] = row[t];
  if (lane == 1 && controls) {
    // detokenize: half = (token_nums - 4) / 2, strict comparisons, brake = -acc
    const double half = (double)(a.token_nums - 4) / 2.0;
    const long long t0 = row[a.first], t1 = row[a.first + 1], t2 = row[a.first + 2];
    const double acc = (double)t0 / half - 1.0;
    const bool fwd = (double)t0 > half;
    double *o = controls + (long long)b * 4;
    o[0] = fwd ? acc : 0.0;
    o[1] = fwd ? 0.0 : -acc;
    o[2] = (double)t1 / half - 1.0;
    o[3] = (double)t2 > half ? 1.0 : 0.0;
  }
}

// B * 3 elements
__global__ void __launch_bounds__(64)
    k_target_select(const float *__restrict__ state, const float *__restrict__ goal, int n,
                    float *__restrict__ target) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int b = i / 3, j = i - b * 3;
  target[i] = (j < 2 && state[b * 3] != 0.f) ? state[b * 3 + 1 + j] : goal[i];
}

static int slot_shape_check(int B, int X, int Y, const char *who) {
  E2EP_REQUIRE(B > 0 && X > 0 && Y > 0, E2EP_EINVAL, "%s: bad shape (B=%d X=%d Y=%d)", who, B, X, Y);
  E2EP_REQUIRE(B <= 65535, E2EP_ERANGE, "%s: B=%d exceeds the grid (65535)", who, B);
  // the per-workgroup partials are int32: X * Y * max(X, Y) bounds every sum
  const long long xy = (long long)X * Y;
  E2EP_REQUIRE(xy <= 0x7fffffffLL && xy * (X > Y ? X : Y) <= 0x7fffffffLL, E2EP_ERANGE,
               "%s: X * Y * max(X, Y) of a %d x %d map does not fit int32", who, X, Y);
  return 0;
}

}  // namespace e2ep

using namespace e2ep;

extern "C" {

size_t e2ep_slot_stats_workspace(int B, int X) {
  if (B <= 0 || X <= 0) return 0;
  return (size_t)B * slot_bands(X) * 3 * sizeof(int);
}

int e2ep_slot_partials(const float *logits, long long stride_b, long long stride_c,
                       long long stride_x, long long stride_y, int B, int C, int X, int Y,
                       int target_class, const unsigned char *class_lut, void *class_image,
                       void *workspace, size_t workspace_bytes, void *stream) {
  E2EP_REQUIRE(logits && workspace, E2EP_EINVAL, "e2ep_slot_partials: null buffer");
  E2EP_REQUIRE(C >= 2 && C <= AG_MAX_C, E2EP_EINVAL, "e2ep_slot_partials: C=%d outside 2..%d", C,
               AG_MAX_C);
  E2EP_REQUIRE(target_class >= 0 && target_class < C, E2EP_EINVAL,
               "e2ep_slot_partials: target_class %d outside [0, %d)", target_class, C);
  if (int rc = slot_shape_check(B, X, Y, "e2ep_slot_partials")) return rc;
  E2EP_REQUIRE(stride_b >= 0 && stride_c > 0 && stride_x > 0 && stride_y > 0, E2EP_EINVAL,
               "e2ep_slot_partials: strides must be positive");
  E2EP_REQUIRE(!class_image || class_lut, E2EP_EINVAL,
               "e2ep_slot_partials: a class image needs its lookup table");
  E2EP_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)workspace & 3) == 0, E2EP_EINVAL,
               "e2ep_slot_partials: misaligned buffer");
  E2EP_REQUIRE(workspace_bytes >= e2ep_slot_stats_workspace(B, X), E2EP_EINVAL,
               "e2ep_slot_partials: workspace %zu < %zu bytes", workspace_bytes,
               e2ep_slot_stats_workspace(B, X));
  SlotArgs a;
  a.C = C, a.X = X, a.Y = Y, a.rows = slot_band_rows(X);
  a.sb = stride_b, a.sc = stride_c, a.sx = stride_x, a.sy = stride_y;
  a.target = target_class;
  a.lut = 0;
  if (class_lut)
    for (int k = 0; k < C; ++k) a.lut |= (unsigned long long)class_lut[k] << (8 * k);
  const bool vec = stride_y == 1 && Y % 4 == 0 && ((uintptr_t)logits & 15) == 0 &&
                   stride_b % 4 == 0 && stride_c % 4 == 0 && stride_x % 4 == 0 &&
                   ((uintptr_t)class_image & 3) == 0;
  const dim3 grid(slot_bands(X), B), block(AG_THREADS);
  int *part = static_cast<int *>(workspace);
  unsigned char *img = static_cast<unsigned char *>(class_image);
  if (vec)
    hipLaunchKernelGGL(k_slot_partials<true>, grid, block, 0, as_stream(stream), logits, a, part, img);
  else
    hipLaunchKernelGGL(k_slot_partials<false>, grid, block, 0, as_stream(stream), logits, a, part, img);
  return launch_status("e2ep_slot_partials");
}

int e2ep_slot_finish(const void *workspace, size_t workspace_bytes, int B, int X, int Y,
                     double res_x, double res_y, float *state, int32_t *found, int64_t *stats,
                     const int64_t *seq, int seq_stride, int seq_len, int first, int token_nums,
                     double *controls, int64_t *tokens_out, void *stream) {
  E2EP_REQUIRE(workspace && state, E2EP_EINVAL, "e2ep_slot_finish: null buffer");
  if (int rc = slot_shape_check(B, X, Y, "e2ep_slot_finish")) return rc;
  E2EP_REQUIRE(workspace_bytes >= e2ep_slot_stats_workspace(B, X), E2EP_EINVAL,
               "e2ep_slot_finish: workspace %zu < %zu bytes", workspace_bytes,
               e2ep_slot_stats_workspace(B, X));
  E2EP_REQUIRE(!seq || ((controls || tokens_out) && seq_len > 0 && seq_stride >= seq_len &&
                        first >= 0 && first + 3 <= seq_len && token_nums > 4),
               E2EP_EINVAL, "e2ep_slot_finish: bad token row (stride %d, length %d, first %d, "
               "token_nums %d)", seq_stride, seq_len, first, token_nums);
  E2EP_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)stats & 7) == 0 &&
                   ((uintptr_t)seq & 7) == 0 && ((uintptr_t)controls & 7) == 0 &&
                   ((uintptr_t)tokens_out & 7) == 0,
               E2EP_EINVAL, "e2ep_slot_finish: misaligned buffer");
  FinishArgs a;
  a.bands = slot_bands(X), a.X = X;
  a.res_x = res_x, a.res_y = res_y;
  a.seq = reinterpret_cast<const long long *>(seq);
  a.seq_stride = seq_stride, a.seq_len = seq_len, a.first = first, a.token_nums = token_nums;
  hipLaunchKernelGGL(k_slot_finish, dim3(B), dim3(64), 0, as_stream(stream),
                     static_cast<const int *>(workspace), a, state, found,
                     reinterpret_cast<long long *>(stats), controls,
                     reinterpret_cast<long long *>(tokens_out));
  return launch_status("e2ep_slot_finish");
}

int e2ep_target_select(const float *state, const float *goal, int B, float *target,
                       void *stream) {
  E2EP_REQUIRE(state && goal && target, E2EP_EINVAL, "e2ep_target_select: null buffer");
  E2EP_REQUIRE(B > 0 && B <= 0x7fffffff / 3, E2EP_EINVAL, "e2ep_target_select: bad B=%d", B);
  hipLaunchKernelGGL(k_target_select, dim3(cdiv((long long)B * 3, 64)), dim3(64), 0,
                     as_stream(stream), state, goal, B * 3, target);
  return launch_status("e2ep_target_select");
}

}  // extern "C"
