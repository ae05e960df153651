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
#include "common.h"

namespace e2ep {

constexpr int DEC_THREADS = 256;

__device__ __forceinline__ unsigned byte_of(const unsigned w[3], int k) {
  return (w[k >> 2] >> ((k & 3) * 8)) & 0xffu;
}

// torchvision ToTensor + Normalize of one uint8 value of channel c (0 = R): / 255, minus the
// ImageNet mean, over the ImageNet std, three fp32 roundings in that order.  The one statement
// of this arithmetic: the cached-crop decode and the raw BGRA decode both call it.
__device__ __forceinline__ float normalise_u8(unsigned byte, int c) {
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  return ((float)byte / 255.f - mean[c]) / stdv[c];
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
  if (depth_rgb) {
    const unsigned w[3] = {depth_rgb[3 * sq], depth_rgb[3 * sq + 1], depth_rgb[3 * sq + 2]};
    double d[4];
    for (int j = 0; j < 4; ++j) {
      // exact integer sum, then the reference's two float64 roundings: / (2^24 - 1), * 1000
      const double s = (double)(byte_of(w, 3 * j) + 256u * byte_of(w, 3 * j + 1) +
                                65536u * byte_of(w, 3 * j + 2));
      d[j] = 1000.0 * (s / 16777215.0);
    }
    double2 *o = reinterpret_cast<double2 *>(depth + frame * hw + off);
    o[0] = make_double2(d[0], d[1]);
    o[1] = make_double2(d[2], d[3]);
  }
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
