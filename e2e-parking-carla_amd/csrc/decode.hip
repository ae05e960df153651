// Frame decode: the per-step arithmetic of the reference data path, on the GPU.
//
// The reference decodes every camera frame on the CPU each step (dataset/carla_dataset.py):
//   image  ProcessImage (:494-515): uint8 RGB crop -> fp32 / 255 -> minus ImageNet mean ->
//          over ImageNet std (torchvision ToTensor + Normalize), channels-first;
//   depth  get_depth (:114-131): uint8 CARLA depth RGB -> (R + 256 G + 65536 B) / (2^24 - 1)
//          * 1000, float64 metres;
//   seg    (:404-406) class map -> int64.
// The frame cache (dataset/frame_cache.py) keeps the cropped uint8 pixels resident in HBM;
// these kernels gather a batch out of it (optional source-frame / source-row table) and turn
// it into the reference's tensors in the same pass.  HBM-bound byte work:
// one thread per 4 pixels (3 dword loads of packed RGB, float4 / double2 stores), 26 bytes
// of traffic per camera pixel (6 read, 12 + 8 written).
//
// The closed-loop agent has no cache: its frames arrive as raw BGRA sensor bytes
// (agent/parking_agent.py:458-465, four ProcessImage calls per tick).  k_decode_bgra crops
// and normalises them straight from the uploaded bytes with the same arithmetic.
//
// Photometric augmentation (k_decode_frames_aug) jitters the image between the / 255 and the
// normalisation, in registers, from counter-based draws; its statement is at the kernel.
#include "common.h"
#include "mix64.h"

namespace e2ep {

constexpr int DEC_THREADS = 256;

__device__ __forceinline__ unsigned byte_of(const unsigned w[3], int k) {
  return (w[k >> 2] >> ((k & 3) * 8)) & 0xffu;
}

// torchvision Normalize of one value x in [0, 1] of channel c (0 = R): minus the ImageNet
// mean, over the ImageNet std, two fp32 roundings in that order.
__device__ __forceinline__ float normalise_unit(float x, int c) {
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  return (x - mean[c]) / stdv[c];
}

// torchvision ToTensor + Normalize of one uint8 value of channel c: / 255, then
// normalise_unit, three fp32 roundings in all.  The one statement of this arithmetic: the
// cached-crop decode, the augmented decode and the raw BGRA decode all go through it.
__device__ __forceinline__ float unit_u8(unsigned byte) { return (float)byte / 255.f; }
__device__ __forceinline__ float normalise_u8(unsigned byte, int c) {
  return normalise_unit(unit_u8(byte), c);
}

// CARLA depth of the 4 pixels of source quad sq -> float64 metres at dst (16-byte aligned).
__device__ __forceinline__ void decode_depth_quad(const unsigned *__restrict__ depth_rgb,
                                                  long long sq, double *__restrict__ dst) {
  const unsigned w[3] = {depth_rgb[3 * sq], depth_rgb[3 * sq + 1], depth_rgb[3 * sq + 2]};
  double d[4];
  for (int j = 0; j < 4; ++j) {
    // exact integer sum, then the reference's two float64 roundings: / (2^24 - 1), * 1000
    const double s = (double)(byte_of(w, 3 * j) + 256u * byte_of(w, 3 * j + 1) +
                              65536u * byte_of(w, 3 * j + 2));
    d[j] = 1000.0 * (s / 16777215.0);
  }
  double2 *o = reinterpret_cast<double2 *>(dst);
  o[0] = make_double2(d[0], d[1]);
  o[1] = make_double2(d[2], d[3]);
}

// rgb/depth_rgb [*][hw][3] uint8 (either may be null); output frame f reads source frame
// src[f] (f when src is null); image [frames][3][hw] fp32; depth [frames][hw] fp64.
// hw % 4 == 0, so a quad never straddles two frames.
__global__ void __launch_bounds__(DEC_THREADS)
    k_decode_frames(const unsigned *__restrict__ rgb, const unsigned *__restrict__ depth_rgb,
                    const long long *__restrict__ src, long long quads, int hw,
                    float *__restrict__ image, double *__restrict__ depth) {
  const long long q = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
  if (q >= quads) return;
  const long long p0 = q * 4;
  const long long frame = p0 / hw;
  const int off = (int)(p0 - frame * hw);
  // source quad: 3 dwords per quad, hw / 4 quads per frame
  const long long sq = (src ? src[frame] : frame) * (hw / 4) + off / 4;
  if (rgb) {
    const unsigned w[3] = {rgb[3 * sq], rgb[3 * sq + 1], rgb[3 * sq + 2]};
    for (int c = 0; c < 3; ++c) {
      float v[4];
      for (int j = 0; j < 4; ++j) v[j] = normalise_u8(byte_of(w, 3 * j + c), c);
      *reinterpret_cast<float4 *>(image + (frame * 3 + c) * hw + off) =
          make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  if (depth_rgb) decode_depth_quad(depth_rgb, sq, depth + frame * hw + off);
}

// Photometric augmentation, a pure function of (seed, epoch, frame key, pixel, bytes); the
// NumPy statement of the same function is tests/augment_ref.py.
//   Draws.  base = mix64(seed ^ mix64(epoch)) comes from the host.  Output frame f has the
//   int64 key key[f]; fh = mix64(base + key[f]); parameter j draws
//   u_j = float(mix64(fh + j) >> 40) * 2^-24 (j = 0 brightness, 1 contrast, 2 saturation,
//   3 grey).
//   Factors (fp32, every operation rounded): b = 1 + B (2 u0 - 1), c = 1 + C (2 u1 - 1),
//   s = 1 + S (2 u2 - 1), and s = 0 when u3 < gray_p.
//   Pivot.  m = gray_mean[f]: the grey mean of the unjittered source frame
//   (k_frame_gray_finish), so k = (1 - c) m.
//   Per pixel, from x_c = float(byte_c) / 255, with clamp(x) = min(max(x, 0), 1):
//     1. brightness  x_c = clamp(x_c b)
//     2. contrast    x_c = clamp(c x_c + k)
//     3. saturation  g = (0.299 x_R + 0.587 x_G) + 0.114 x_B;  x_c = clamp(s x_c + (1 - s) g)
//     4. noise       h = mix64(fh ^ mix64(p)), p the pixel's index within its frame; channel
//                    c draws u = float((h >> 21 c) & 0x1FFFFF) * 2^-21;
//                    x_c = clamp(x_c + a (2 u - 1))
//     5. normalise_unit(x_c, c).
// No contraction (this file is built -ffp-contract=off).  With B = C = S = a = gray_p = 0
// steps 1-4 are the identity bit for bit, so the result is k_decode_frames'.
struct PhotoAug {
  unsigned long long base;
  float B, C, S, noise, gray_p;
};

__device__ __forceinline__ float clamp_unit(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float draw24(unsigned long long h) {
  return (float)(h >> 40) * 0x1p-24f;
}

// k_decode_frames' thread-to-quad map, loads and stores; key [frames] int64 and gray_mean
// [frames] fp32 are read only when rgb is not null.  A quad never straddles two frames, so
// the frame's factors are computed once per thread.
__global__ void __launch_bounds__(DEC_THREADS)
    k_decode_frames_aug(const unsigned *__restrict__ rgb, const unsigned *__restrict__ depth_rgb,
                        const long long *__restrict__ src, const long long *__restrict__ key,
                        const float *__restrict__ gray_mean, PhotoAug a, long long quads, int hw,
                        float *__restrict__ image, double *__restrict__ depth) {
  const long long q = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
  if (q >= quads) return;
  const long long p0 = q * 4;
  const long long frame = p0 / hw;
  const int off = (int)(p0 - frame * hw);
  const long long sq = (src ? src[frame] : frame) * (hw / 4) + off / 4;
  if (rgb) {
    const unsigned long long fh = mix64(a.base + (unsigned long long)key[frame]);
    const float fb = 1.f + a.B * (2.f * draw24(mix64(fh)) - 1.f);
    const float fc = 1.f + a.C * (2.f * draw24(mix64(fh + 1)) - 1.f);
    float fs = 1.f + a.S * (2.f * draw24(mix64(fh + 2)) - 1.f);
    if (draw24(mix64(fh + 3)) < a.gray_p) fs = 0.f;
    const float k = (1.f - fc) * gray_mean[frame];
    const float t = 1.f - fs;
    const unsigned w[3] = {rgb[3 * sq], rgb[3 * sq + 1], rgb[3 * sq + 2]};
    float v[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = clamp_unit(unit_u8(byte_of(w, 3 * j + c)) * fb);
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = clamp_unit(fc * x[c] + k);
      const float grey = (0.299f * x[0] + 0.587f * x[1]) + 0.114f * x[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = clamp_unit(fs * x[c] + t * grey);
      const unsigned long long h = mix64(fh ^ mix64((unsigned long long)(off + j)));
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float u = (float)((unsigned)(h >> (21 * c)) & 0x1FFFFFu) * 0x1p-21f;
        x[c] = clamp_unit(x[c] + a.noise * (2.f * u - 1.f));
        v[c][j] = normalise_unit(x[c], c);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<float4 *>(image + (frame * 3 + c) * hw + off) =
          make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
  }
  if (depth_rgb) decode_depth_quad(depth_rgb, sq, depth + frame * hw + off);
}

// Exact channel sums of the source frames: sums [frames][3] int64 (zeroed before the launch)
// += the R, G, B byte sums of source frame src[f].  A frame is spread over `parts` blocks
// (blockIdx.x = f * parts + part), each striding over the frame's quads with the decode's
// dword loads; per-thread uint32 partials (at most 2^15 quads of 4 x 255 per thread), a wave
// shuffle, one LDS step and one 64-bit integer atomic per block and channel: integer
// addition makes every order exact.
__global__ void __launch_bounds__(DEC_THREADS)
    k_frame_channel_sums(const unsigned *__restrict__ rgb, const long long *__restrict__ src,
                         int parts, int hw, unsigned long long *__restrict__ sums) {
  const long long frame = blockIdx.x / parts;
  const int part = blockIdx.x - (int)frame * parts;
  const int qpf = hw / 4;
  const unsigned *base = rgb + (src ? src[frame] : frame) * qpf * 3;
  unsigned acc[3] = {0u, 0u, 0u};
  for (int i = part * DEC_THREADS + threadIdx.x; i < qpf; i += parts * DEC_THREADS) {
    const unsigned w[3] = {base[3 * (long long)i], base[3 * (long long)i + 1],
                           base[3 * (long long)i + 2]};
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k % 3] += byte_of(w, k);
  }
  __shared__ unsigned part_sum[DEC_THREADS / 64][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
    if ((threadIdx.x & 63) == 0) part_sum[threadIdx.x >> 6][c] = acc[c];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long s = 0;
    for (int wv = 0; wv < DEC_THREADS / 64; ++wv) s += part_sum[wv][threadIdx.x];
    atomicAdd(sums + frame * 3 + threadIdx.x, s);
  }
}

// mean[f] = float32((0.299 sumR + 0.587 sumG + 0.114 sumB) / (255 hw)), the sum left to right
// in float64 and one rounding to fp32: the contrast pivot of k_decode_frames_aug.
__global__ void k_frame_gray_finish(const long long *__restrict__ sums, long long frames, int hw,
                                    float *__restrict__ mean) {
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= frames) return;
  const double r = (double)sums[3 * f], g = (double)sums[3 * f + 1], b = (double)sums[3 * f + 2];
  mean[f] = (float)(((0.299 * r + 0.587 * g) + 0.114 * b) / (255.0 * (double)hw));
}

// Raw sensor frames: bgra [N][H][W] dwords (B, G, R, A bytes: a CARLA image's raw_data), the
// centred crop x crop window at (top, left) -> image [N][3][crop][crop] fp32 normalised and,
// when rgb is not null, the uint8 crop [N][crop][crop][3].  One thread per V consecutive
// pixels of a crop row: V dword loads (a pixel is one aligned dword), then per channel one
// V-float store and V * 3 packed RGB bytes, all contiguous along the row across the wave.
// V = 4 needs crop % 4 == 0 (16-byte image stores, dword RGB stores); V = 1 is the general path.
template <int V>
__global__ void __launch_bounds__(DEC_THREADS)
    k_decode_bgra(const unsigned *__restrict__ bgra, long long groups, int H, int W, int crop,
                  int top, int left, float *__restrict__ image,
                  unsigned char *__restrict__ rgb) {
  const long long g = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
  if (g >= groups) return;
  const int gpr = crop / V;  // groups per crop row
  const long long row = g / gpr;
  const int c0 = (int)(g - row * gpr) * V;
  const long long n = row / crop;
  const int r = (int)(row - n * crop);
  const unsigned *src = bgra + (n * H + top + r) * W + left + c0;
  unsigned w[V];
#pragma unroll
  for (int j = 0; j < V; ++j) w[j] = src[j];
  const long long plane = (long long)crop * crop;
  const long long o = (long long)r * crop + c0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = normalise_u8((w[j] >> (8 * (2 - c))) & 0xffu, c);
    float *dst = image + (n * 3 + c) * plane + o;
    if constexpr (V == 4) {
      *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      dst[0] = v[0];
    }
  }
  if (!rgb) return;
  unsigned char *out = rgb + (n * plane + o) * 3;
  if constexpr (V == 4) {
    // 12 bytes R G B R G B ... from four B G R A dwords
    unsigned p[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const unsigned b = (w[k / 3] >> (8 * (2 - k % 3))) & 0xffu;
      p[k >> 2] |= b << ((k & 3) * 8);
    }
    unsigned *o32 = reinterpret_cast<unsigned *>(out);
    o32[0] = p[0];
    o32[1] = p[1];
    o32[2] = p[2];
  } else {
    out[0] = (unsigned char)((w[0] >> 16) & 0xffu);
    out[1] = (unsigned char)((w[0] >> 8) & 0xffu);
    out[2] = (unsigned char)(w[0] & 0xffu);
  }
}

// uint8 rows -> int64 (class maps): output row r reads source row src[r] (r when null);
// 4 bytes per thread, one dword load, two 16-byte stores.  row_len % 4 == 0.
__global__ void __launch_bounds__(DEC_THREADS)
    k_widen_u8_i64(const unsigned *__restrict__ in, const long long *__restrict__ src,
                   long long quads, int row_len, long long *__restrict__ dst) {
  const long long q = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
  if (q >= quads) return;
  const long long row = q * 4 / row_len;
  const int off = (int)(q * 4 - row * row_len);
  const unsigned w = in[((src ? src[row] : row) * row_len + off) / 4];
  longlong2 *o = reinterpret_cast<longlong2 *>(dst + q * 4);
  o[0] = make_longlong2(w & 0xff, (w >> 8) & 0xff);
  o[1] = make_longlong2((w >> 16) & 0xff, w >> 24);
}

}  // namespace e2ep

using namespace e2ep;

extern "C" {

int e2ep_decode_frames(const void *rgb, const void *depth_rgb, const long long *src_frame,
                       long long frames, int hw, float *image, double *depth, void *stream) {
  E2EP_REQUIRE(frames >= 0 && hw > 0 && hw % 4 == 0, E2EP_EINVAL,
               "e2ep_decode_frames: need hw %% 4 == 0 (hw=%d)", hw);
  E2EP_REQUIRE((!rgb || image) && (!depth_rgb || depth), E2EP_EINVAL,
               "e2ep_decode_frames: missing output");
  E2EP_REQUIRE(((uintptr_t)rgb & 3) == 0 && ((uintptr_t)depth_rgb & 3) == 0 &&
                   ((uintptr_t)image & 15) == 0 && ((uintptr_t)depth & 15) == 0,
               E2EP_EINVAL, "e2ep_decode_frames: misaligned buffer");
  const long long quads = frames * hw / 4;
  if (quads == 0 || (!rgb && !depth_rgb)) return 0;
  hipLaunchKernelGGL(k_decode_frames, dim3(cdiv(quads, DEC_THREADS)), dim3(DEC_THREADS), 0,
                     as_stream(stream), static_cast<const unsigned *>(rgb),
                     static_cast<const unsigned *>(depth_rgb), src_frame, quads, hw, image, depth);
  return launch_status("e2ep_decode_frames");
}

int e2ep_frame_gray_mean(const void *rgb, const long long *src_frame, long long frames, int hw,
                         long long *sums, float *mean, void *stream) {
  E2EP_REQUIRE(frames >= 0 && hw > 0 && hw % 4 == 0, E2EP_EINVAL,
               "e2ep_frame_gray_mean: need hw %% 4 == 0 (hw=%d)", hw);
  if (frames == 0) return 0;
  E2EP_REQUIRE(rgb && sums && mean, E2EP_EINVAL, "e2ep_frame_gray_mean: null buffer");
  E2EP_REQUIRE(((uintptr_t)rgb & 3) == 0 && ((uintptr_t)sums & 7) == 0 &&
                   ((uintptr_t)mean & 3) == 0,
               E2EP_EINVAL, "e2ep_frame_gray_mean: misaligned buffer");
  // 8 quads per thread until 64 blocks share a frame: 8 blocks per 256 x 256 frame
  int parts = cdiv(hw / 4, DEC_THREADS * 8);
  parts = parts < 1 ? 1 : parts > 64 ? 64 : parts;
  E2EP_REQUIRE(frames * parts <= 0x7fffffffLL, E2EP_ERANGE,
               "e2ep_frame_gray_mean: %lld frames exceed one grid", frames);
  hipStream_t s = as_stream(stream);
  hipError_t e = hipMemsetAsync(sums, 0, (size_t)frames * 3 * sizeof(long long), s);
  E2EP_REQUIRE(e == hipSuccess, (int)e, "e2ep_frame_gray_mean: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_frame_channel_sums, dim3((unsigned)(frames * parts)), dim3(DEC_THREADS), 0,
                     s, static_cast<const unsigned *>(rgb), src_frame, parts, hw,
                     reinterpret_cast<unsigned long long *>(sums));
  hipLaunchKernelGGL(k_frame_gray_finish, dim3(cdiv(frames, DEC_THREADS)), dim3(DEC_THREADS), 0,
                     s, sums, frames, hw, mean);
  return launch_status("e2ep_frame_gray_mean");
}

int e2ep_decode_frames_aug(const void *rgb, const void *depth_rgb, const long long *src_frame,
                           const long long *frame_key, long long frames, int hw,
                           const float *gray_mean, long long base, float B, float C, float S,
                           float noise, float gray_p, float *image, double *depth,
                           void *stream) {
  E2EP_REQUIRE(frames >= 0 && hw > 0 && hw % 4 == 0, E2EP_EINVAL,
               "e2ep_decode_frames_aug: need hw %% 4 == 0 (hw=%d)", hw);
  E2EP_REQUIRE(B >= 0.f && B <= 1.f && C >= 0.f && C <= 1.f && S >= 0.f && S <= 1.f &&
                   noise >= 0.f && noise <= 0.5f && gray_p >= 0.f && gray_p <= 1.f,
               E2EP_EINVAL,
               "e2ep_decode_frames_aug: brightness, contrast, saturation and gray_p lie in "
               "[0, 1], noise in [0, 0.5]");
  const long long quads = frames * hw / 4;
  if (quads == 0) return 0;
  E2EP_REQUIRE(rgb && image && frame_key && gray_mean && (!depth_rgb || depth), E2EP_EINVAL,
               "e2ep_decode_frames_aug: null buffer");
  E2EP_REQUIRE(((uintptr_t)rgb & 3) == 0 && ((uintptr_t)depth_rgb & 3) == 0 &&
                   ((uintptr_t)image & 15) == 0 && ((uintptr_t)depth & 15) == 0 &&
                   ((uintptr_t)frame_key & 7) == 0 && ((uintptr_t)gray_mean & 3) == 0,
               E2EP_EINVAL, "e2ep_decode_frames_aug: misaligned buffer");
  const PhotoAug a = {(unsigned long long)base, B, C, S, noise, gray_p};
  hipLaunchKernelGGL(k_decode_frames_aug, dim3(cdiv(quads, DEC_THREADS)), dim3(DEC_THREADS), 0,
                     as_stream(stream), static_cast<const unsigned *>(rgb),
                     static_cast<const unsigned *>(depth_rgb), src_frame, frame_key, gray_mean, a,
                     quads, hw, image, depth);
  return launch_status("e2ep_decode_frames_aug");
}

int e2ep_decode_bgra(const void *bgra, int N, int H, int W, int crop, float *image, void *rgb,
                     void *stream) {
  E2EP_REQUIRE(bgra && image, E2EP_EINVAL, "e2ep_decode_bgra: null buffer");
  E2EP_REQUIRE(N > 0 && H > 0 && W > 0 && crop > 0, E2EP_EINVAL,
               "e2ep_decode_bgra: bad shape (N=%d H=%d W=%d crop=%d)", N, H, W, crop);
  E2EP_REQUIRE(crop <= H && crop <= W, E2EP_EINVAL,
               "e2ep_decode_bgra: crop %d larger than the %d x %d frame", crop, H, W);
  E2EP_REQUIRE(((uintptr_t)bgra & 3) == 0 && ((uintptr_t)image & 3) == 0, E2EP_EINVAL,
               "e2ep_decode_bgra: misaligned buffer");
  const int top = H / 2 - crop / 2, left = W / 2 - crop / 2;
  const bool quad = crop % 4 == 0 && ((uintptr_t)image & 15) == 0 && ((uintptr_t)rgb & 3) == 0;
  const long long groups = (long long)N * crop * (crop / (quad ? 4 : 1));
  E2EP_REQUIRE(groups <= 0x7fffffffLL * DEC_THREADS, E2EP_ERANGE,
               "e2ep_decode_bgra: %lld pixel groups exceed one grid", groups);
  const dim3 grid(cdiv(groups, DEC_THREADS)), block(DEC_THREADS);
  const unsigned *src = static_cast<const unsigned *>(bgra);
  unsigned char *out = static_cast<unsigned char *>(rgb);
  if (quad)
    hipLaunchKernelGGL(k_decode_bgra<4>, grid, block, 0, as_stream(stream), src, groups, H, W,
                       crop, top, left, image, out);
  else
    hipLaunchKernelGGL(k_decode_bgra<1>, grid, block, 0, as_stream(stream), src, groups, H, W,
                       crop, top, left, image, out);
  return launch_status("e2ep_decode_bgra");
}

int e2ep_widen_u8_i64(const void *src, const long long *src_row, long long rows, int row_len,
                      long long *dst, void *stream) {
  E2EP_REQUIRE(rows >= 0 && row_len > 0 && row_len % 4 == 0, E2EP_EINVAL,
               "e2ep_widen_u8_i64: need row_len %% 4 == 0 (row_len=%d)", row_len);
  E2EP_REQUIRE(rows == 0 || (src && dst), E2EP_EINVAL, "e2ep_widen_u8_i64: null buffer");
  E2EP_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 15) == 0, E2EP_EINVAL,
               "e2ep_widen_u8_i64: misaligned buffer");
  const long long quads = rows * row_len / 4;
  if (quads == 0) return 0;
  hipLaunchKernelGGL(k_widen_u8_i64, dim3(cdiv(quads, DEC_THREADS)), dim3(DEC_THREADS), 0,
                     as_stream(stream), static_cast<const unsigned *>(src), src_row, quads,
                     row_len, dst);
  return launch_status("e2ep_widen_u8_i64");
}

}  // extern "C"
