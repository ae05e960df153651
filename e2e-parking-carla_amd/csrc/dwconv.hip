// Depthwise (groups == channels, multiplier 1) conv for EfficientNet's MBConv
// (efficientnet-pytorch 0.7.1 _depthwise_conv: k3/k5, stride 1/2, static SAME padding),
// forward, data gradient (gather, no atomics) and weight gradient (fixed-order split
// reduction), NCHW fp32, for gfx950.  Memory-bound: each kernel streams its input once.
#include <type_traits>

#include "common.h"
#include "handoff.h"

// Contraction only within one expression (a*b + c -> fma): the fp32 and bf16-storage
// instantiations of a kernel (E2EP_IO_*) then fuse the same operations and round alike —
// under the default cross-statement contraction hipcc may pick a different multiply to fuse
// in each instantiation (tests/test_bf16_store_gpu.py holds them bitwise equal).
#pragma clang fp contract(on)

namespace e2ep {

// Weight-gradient output: per-split slabs part[c][split][K*K]; with one split the slab is the
// gradient and is written to dw directly; with several and `cnt` (the in-launch fold, e2ep_tune
// key 28 = 2) the slabs are stored write-through and the channel's last-arriving split sums
// them in split order (k_dw_wgrad_finalize's order) into dw; otherwise k_dw_wgrad_finalize does.
struct DwPart {
  float *part, *dw;
  unsigned int *cnt;
};

template <int KK>
__device__ __forceinline__ void dw_wgrad_out(DwPart o, int c, int sp, int splits, float v,
                                             int *s_last) {
  const int t = threadIdx.x;
  if (t < KK) {
    if (splits == 1) o.dw[(long long)c * KK + t] = v;
    else if (o.cnt) st_sc1(o.part + ((long long)c * splits + sp) * KK + t, v);
    else o.part[((long long)c * splits + sp) * KK + t] = v;
  }
  if (splits == 1 || !o.cnt) return;
  handoff_drain();
  if (!handoff_arrive(o.cnt + c, splits, s_last)) return;
  if (t < KK) {
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += ld_sc1(o.part + ((long long)c * splits + k) * KK + t);
    o.dw[(long long)c * KK + t] = s;
  }
}

struct DwGeom {
  int N, C, H, W, K, P, Q, st, pt, pl;
};

// Optional input transform of the forward / weight-gradient kernels: the input is the raw
// output of the preceding 1x1 conv and the kernel applies that layer's BatchNorm (per-channel
// scale / shift from e2ep_bn_stats) and activation on load, so the normalised tensor is never
// written (zero padding stays zero: it lives in the normalised space).
struct DwIn {
  const float *sc, *sh;  // [C] or null (identity)
  int act;               // 0 none, 1 relu, 2 swish
};
__device__ __forceinline__ float dw_in(float v, float sc, float sh, int act) {
  const float z = v * sc + sh;
  return act == 2 ? swish_f(z) : act == 1 ? fmaxf(z, 0.f) : z;
}

// forward: one thread per output pixel; taps unrolled; branch-free guarded loads
template <int K, int ST>
__global__ void __launch_bounds__(256) k_dw_fwd(const float *__restrict__ x,
                                                const float *__restrict__ w, DwGeom g,
                                                float *__restrict__ y, const float *__restrict__ tsc,
                                                const float *__restrict__ tsh, int tact) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.P * g.Q) return;
  const int nc = blockIdx.y;
  const int c = nc % g.C;
  const int oy = i / g.Q, ox = i - oy * g.Q;
  const int HW = g.H * g.W;
  const __amdgpu_buffer_rsrc_t rx = rsrc(x + (size_t)nc * HW, 4LL * HW);
  const float *wp = w + c * K * K;
  const int y0 = oy * ST - g.pt, x0 = ox * ST - g.pl;
  float v[K * K];
#pragma unroll
  for (int a = 0; a < K; ++a) {
    const int iy = y0 + a;
#pragma unroll
    for (int b = 0; b < K; ++b) {
      const int ix = x0 + b;
      const bool ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
      v[a * K + b] = bload(rx, ok ? (iy * g.W + ix) * 4 : OOR);
      if (tsc && ok) v[a * K + b] = dw_in(v[a * K + b], tsc[c], tsh[c], tact);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < K * K; ++t) s += wp[t] * v[t];
  y[(size_t)nc * g.P * g.Q + i] = s;
}

// data gradient: one thread per input pixel, gather the outputs whose window covers it
// (branch-free: invalid taps read 0 through an out-of-range buffer offset)
template <int K, int ST>
__global__ void __launch_bounds__(256) k_dw_dgrad(const float *__restrict__ gy,
                                                  const float *__restrict__ w, DwGeom g,
                                                  float *__restrict__ dx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.H * g.W) return;
  const int nc = blockIdx.y;
  const int c = nc % g.C;
  const int iy = i / g.W, ix = i - iy * g.W;
  const int PQ = g.P * g.Q;
  const __amdgpu_buffer_rsrc_t rg = rsrc(gy + (size_t)nc * PQ, 4LL * PQ);
  const float *wp = w + c * K * K;
  float v[K * K];
#pragma unroll
  for (int a = 0; a < K; ++a) {
    const int ny = iy + g.pt - a;
    const int oy = ny >= 0 ? ny / ST : -1;  // ST is a compile-time 1 or 2
    const bool oky = ny >= 0 && oy * ST == ny && oy < g.P;
#pragma unroll
    for (int b = 0; b < K; ++b) {
      const int nx = ix + g.pl - b;
      const int ox = nx >= 0 ? nx / ST : -1;
      const bool ok = oky && nx >= 0 && ox * ST == nx && ox < g.Q;
      v[a * K + b] = bload(rg, ok ? (oy * g.Q + ox) * 4 : OOR);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < K * K; ++t) s += wp[t] * v[t];
  dx[(size_t)nc * g.H * g.W + i] = s;
}

// weight gradient partials: grid (C, splits); each slice of (n, oy, ox) accumulates K*K taps
template <int K, int ST>
__global__ void __launch_bounds__(256) k_dw_wgrad(const float *__restrict__ gy,
                                                  const float *__restrict__ x, DwGeom g,
                                                  int splits, DwPart part,
                                                  const float *__restrict__ tsc,
                                                  const float *__restrict__ tsh, int tact) {
  const int c = blockIdx.x, sp = blockIdx.y;
  const int PQ = g.P * g.Q;
  const int tot = g.N * PQ;
  const int per = (tot + splits - 1) / splits;
  const int beg = sp * per, end = min(tot, beg + per);
  float acc[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) acc[t] = 0.f;
  const int HW = g.H * g.W;
  const __amdgpu_buffer_rsrc_t rx = rsrc(x, 4LL * g.N * g.C * HW);
  for (int i = beg + threadIdx.x; i < end; i += 256) {
    const int n = i / PQ;
    const int pix = i - n * PQ;
    const int oy = pix / g.Q, ox = pix - oy * g.Q;
    const float gv = gy[((size_t)n * g.C + c) * PQ + pix];
    const int xb = (n * g.C + c) * HW;
    const int y0 = oy * ST - g.pt, x0 = ox * ST - g.pl;
#pragma unroll
    for (int a = 0; a < K; ++a) {
      const int iy = y0 + a;
      const bool oky = (unsigned)iy < (unsigned)g.H;
#pragma unroll
      for (int b = 0; b < K; ++b) {
        const int ix = x0 + b;
        const bool ok = oky && (unsigned)ix < (unsigned)g.W;
        float xv = bload(rx, ok ? (xb + iy * g.W + ix) * 4 : OOR);
        if (tsc && ok) xv = dw_in(xv, tsc[c], tsh[c], tact);
        acc[a * K + b] += gv * xv;
      }
    }
  }
  __shared__ float red[4][K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) {
    const float v = wave_sum(acc[t]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][t] = v;
  }
  __syncthreads();
  const int t = threadIdx.x < K * K ? threadIdx.x : 0;
  // the last-arriver flag reuses red[0][0] (read above, before dw_wgrad_out's first barrier):
  // a static __shared__ int would leave the kernel's static LDS at 4 mod 16 bytes and shift the
  // strip kernels' dynamic LDS base off 16-B alignment (their b128 window reads then replay:
  // 1.5 - 2x slower; cdna_hip_programming.md Guideline 17)
  dw_wgrad_out<K * K>(part, c, sp, splits, (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]),
                      reinterpret_cast<int *>(&red[0][0]));
}

__global__ void k_dw_wgrad_finalize(const float *__restrict__ part, int C, int KK, int splits,
                                    float *__restrict__ dw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C * KK) return;
  const int c = i / KK, t = i - c * KK;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += part[((long long)c * splits + k) * KK + t];
  dw[i] = s;
}

// ------------------------------------------------------------------------------------------
// Strip kernels (Q % 4 == 0, Q <= 256): each wave owns one unit = (plane n*C+c, RO = 256/Q
// consecutive output rows) and every lane 4 horizontally adjacent outputs, so a unit is
// exactly 64 x 4 outputs.  The unit's input rows ((RO-1)*ST + K of them) are staged once in
// LDS with float4 loads, zero-padded left/right (DW_PADL columns) and above/below, and each
// lane reads its (3*ST + K) x K window from LDS: per output K*(3*ST+K)/4 LDS reads instead of
// K*K global loads.  Weights are wave-uniform (scalar loads).  Forward; the stride-1 data
// gradient is the same correlation with the filter flipped and pads K-1-pad (FLIP).
// ------------------------------------------------------------------------------------------
constexpr int DW_PADL = 4;  // left halo columns in LDS (>= max left pad 2, keeps rows 16-B aligned)

struct DwStrip {
  int RO, IR, WP, units_per_plane;  // out rows / unit, staged input rows, LDS row pitch
};

static DwStrip dw_strip(int K, int st, int W, int P, int Q) {
  DwStrip d;
  d.RO = 64 / (Q / 4);  // lanes past RO * (Q / 4) idle
  d.IR = (d.RO - 1) * st + K;
  d.WP = W + 2 * DW_PADL;
  d.units_per_plane = (P + d.RO - 1) / d.RO;
  return d;
}

// Each wave of the strip kernels stages and reads only its own LDS region, so the staging
// needs a wave-level fence, not a block barrier: the wave's LDS writes complete (lgkmcnt(0))
// before any lane reads another lane's words, and the four waves of a block run decoupled.
__device__ __forceinline__ void dw_wave_sync() {
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0); vmcnt / expcnt unconstrained
  __builtin_amdgcn_wave_barrier();
}

// stage input rows [iy0, iy0 + IR) of plane `src` (H x W) into this wave's LDS buffer.  The
// loads are branch-free buffer loads (rows outside the plane read 0 through an out-of-range
// offset) issued before any is used: a guarded `if (row ok) v = load` made hipcc branch
// around each load and wait for it, one round trip per float4 (1.2-3 TB/s, round 3).
constexpr int DW_MAXV = 6;  // float4 per lane the unrolled staging covers (host-checked)
// the input transform resolved for one channel (read once per wave, not per staged row)
struct DwT {
  float sc, sh;
  int act;
  bool on;
};
__device__ __forceinline__ DwT dw_t(DwIn tf, int c) {
  const bool on = tf.sc != nullptr;
  return DwT{on ? tf.sc[c] : 1.f, on ? tf.sh[c] : 0.f, tf.act, on};
}
// transform of one staged float4; `in` = inside the plane (padding stays zero).  The act
// branches are wave-uniform; the padding test is a per-lane select, not a branch
__device__ __forceinline__ float4 dw_tf4(float4 v, const DwT &t, bool in) {
  if (!t.on) return v;
  float z[4] = {v.x * t.sc + t.sh, v.y * t.sc + t.sh, v.z * t.sc + t.sh, v.w * t.sc + t.sh};
  if (t.act == 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = swish_f(z[i]);
  } else if (t.act == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = fmaxf(z[i], 0.f);
  }
  return make_float4(in ? z[0] : 0.f, in ? z[1] : 0.f, in ? z[2] : 0.f, in ? z[3] : 0.f);
}
// buffer descriptor of a wave-uniform plane: the base pointer and size go through
// readfirstlane so the descriptor lives in SGPRs (a VGPR descriptor makes hipcc wrap every
// buffer load in a waterfall loop)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_u(const void *p, long long bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  const int nb = __builtin_amdgcn_readfirstlane((int)(bytes >= 0x7fffffff ? 0x7fffffff : bytes));
  return __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo), (short)0, nb, 0x00020000);
}
template <typename TI>
__device__ __forceinline__ void dw_stage(const TI *__restrict__ src, int H, int W, int iy0,
                                         int IR, int WP, float *lds, int lane,
                                         DwIn tf = DwIn{nullptr, nullptr, 0}, int c = 0) {
  const int W4 = W >> 2;
  const DwT t = dw_t(tf, c);
  constexpr int EB = sizeof(TI);  // bytes per element (4 fp32, 2 bf16 storage)
  const __amdgpu_buffer_rsrc_t rs = rsrc_u(src, (long long)EB * H * W);
  float4 v[DW_MAXV];
  bool in[DW_MAXV];
#pragma unroll
  for (int i = 0; i < DW_MAXV; ++i) {
    const int e = lane + 64 * i;
    const int r = e / W4, j = e - r * W4;
    const int iy = iy0 + r;
    in[i] = e < IR * W4 && (unsigned)iy < (unsigned)H;
    v[i] = bload4t(rs, in[i] ? (iy * W + 4 * j) * EB : OOR, src);
  }
#pragma unroll
  for (int i = 0; i < DW_MAXV; ++i) {
    const int e = lane + 64 * i;
    if (e >= IR * W4) break;
    const int r = e / W4, j = e - r * W4;
    // padding rows stay zero (the padding lives in the normalised space)
    *reinterpret_cast<float4 *>(lds + r * WP + DW_PADL + 4 * j) = dw_tf4(v[i], t, in[i]);
  }
  // halo columns
  for (int e = lane; e < IR * 2 * DW_PADL; e += 64) {
    const int r = e / (2 * DW_PADL), j = e - r * (2 * DW_PADL);
    lds[r * WP + (j < DW_PADL ? j : W + j)] = 0.f;
  }
}

// The same staging split in two for software pipelining: dw_fetch issues a unit's row loads
// into registers (at most DW_MAXV float4 per lane), dw_put writes them (normalised) and the
// halo zeros into LDS once they have landed.
template <int V, typename TI>
__device__ __forceinline__ void dw_fetch(const TI *__restrict__ src, int H, int W, int iy0,
                                         int IR, int lane, float4 (&r)[V], bool active) {
  const int W4 = W >> 2;
  constexpr int EB = sizeof(TI);
  const __amdgpu_buffer_rsrc_t rs = rsrc_u(src, (long long)EB * H * W);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int e = lane + 64 * i;
    const int rr = e / W4, j = e - rr * W4;
    const int iy = iy0 + rr;
    const bool ok = active && e < IR * W4 && (unsigned)iy < (unsigned)H;
    r[i] = bload4t(rs, ok ? (iy * W + 4 * j) * EB : OOR, src);  // branch-free (see dw_stage)
  }
}
template <int V>
__device__ __forceinline__ void dw_put(const float4 (&r)[V], int H, int W, int iy0, int IR,
                                       int WP, float *lds, int lane, const DwT &t) {
  const int W4 = W >> 2;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int e = lane + 64 * i;
    if (e >= IR * W4) break;
    const int rr = e / W4, j = e - rr * W4;
    // padding rows stay zero
    *reinterpret_cast<float4 *>(lds + rr * WP + DW_PADL + 4 * j) =
        dw_tf4(r[i], t, (unsigned)(iy0 + rr) < (unsigned)H);
  }
  for (int e = lane; e < IR * 2 * DW_PADL; e += 64) {
    const int rr = e / (2 * DW_PADL), j = e - rr * (2 * DW_PADL);
    lds[rr * WP + (j < DW_PADL ? j : W + j)] = 0.f;
  }
}

// One lane's LDS window row v[0 .. NV) starting at `base`.  OFF >= 0: base sits OFF floats past a
// 16-B boundary (OFF = -pl mod 4: the staged rows start 16-B aligned, every lane's first
// output column is a multiple of 4), and the row is read as ceil((OFF + NV) / 4) ds_read_b128
// from that boundary: 4 lane groups of 16 consecutive 16-B words, conflict-free, where the
// scalar reads (OFF = -1, e2ep_tune key 23 = 1) land lanes 8 apart on one bank (4-way) at
// 1 or 2 floats per instruction.  The words read past the window stay inside the staged row
// (its right halo), since the row pitch is a multiple of 4.
template <int NV, int OFF>
__device__ __forceinline__ void dw_row(const float *base, float (&v)[NV]) {
  if constexpr (OFF < 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = base[j];
  } else {
    constexpr int NF = (OFF + NV + 3) / 4;
    const float4 *p = reinterpret_cast<const float4 *>(base - OFF);
    float f[4 * NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const float4 t = p[i];
      f[4 * i] = t.x;
      f[4 * i + 1] = t.y;
      f[4 * i + 2] = t.z;
      f[4 * i + 3] = t.w;
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = f[OFF + j];
  }
}

// V: float4 per lane that hold a unit's staged rows (2 or DW_MAXV; the host picks the
// smallest that covers IR * W / 4, so short units keep fewer registers and more waves resident)
// BS: BatchNorm partial sums of y for the BN that follows (MBConv _bn1), one fp64 (sum, sum of
// squares) pair per unit (a lane's 4 outputs in fp32, the wave's 64 lanes in fp64), written by
// the unit's wave, tile-major like bnstats.h: tile = n * units_per_plane + row block,
// stats[(tile * C + c) * 2].
__device__ __forceinline__ double dw_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// bf16 activation storage (B, e2ep.h E2EP_IO_*): the forward's output y (the MBConv depthwise
// output, read by the squeeze-excitation and the _bn1 backward) and, in the backward, the
// incoming gradient gy and the data gradient dx are bf16; the forward's input (the raw expand
// conv output, normalised on load) stays fp32.  FLIP (the stride-1 data gradient) reads gy.
template <bool FLIP, bool B>
using dw_ti = std::conditional_t<FLIP && B, bf16_t, float>;
template <bool B>
using dw_to = std::conditional_t<B, bf16_t, float>;

// The block body for block blk of nblk (k_dw_fwd_strip, and the data-gradient half of
// k_dw_bwd_pair), over the kernel's dynamic LDS.  BS statistics are of the stored (rounded)
// values.
template <int K, int ST, bool FLIP, int OFF, int V, bool BS = false, bool B = false>
__device__ __forceinline__ void dw_fwd_strip_body(const dw_ti<FLIP, B> *__restrict__ x,
                                                  const float *__restrict__ w, DwGeom g, DwStrip d,
                                                  int units, dw_to<B> *__restrict__ y, DwIn tf,
                                                  double *__restrict__ stats, int blk, int nblk) {
  extern __shared__ float dw_lds[];
  // Grid-stride over units, software-pipelined like k_dw_wgrad_strip: the wave's next unit's
  // input rows are loaded into registers before the current unit's FMAs (one unit per wave
  // with stage / wait / compute in series ran at 1.7-3.5 TB/s).  The grid is capped at
  // e2ep_tune key 24 blocks, so each wave walks several units.
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: SGPR descriptors
  float *lds = dw_lds + wave * d.IR * d.WP;
  const int QL = g.Q >> 2;  // lanes per output row
  const int ro = lane / QL, ox0 = 4 * (lane - ro * QL);
  constexpr int NV = 3 * ST + K;
  const int step = nblk * 4;
  int u = blk * 4 + wave;  // wave-uniform
  int nc = 0, oy0 = 0;
  auto unit_of = [&](int un) {
    nc = un / d.units_per_plane;
    oy0 = (un - nc * d.units_per_plane) * d.RO;
  };
  float4 rx[V];
  if (u < units) unit_of(u);
  dw_fetch(x + (size_t)nc * g.H * g.W, g.H, g.W, oy0 * ST - g.pt, d.IR, lane, rx, u < units);
  for (; u < units; u += step) {
    const int c = nc % g.C;
    dw_put(rx, g.H, g.W, oy0 * ST - g.pt, d.IR, d.WP, lds, lane, dw_t(tf, c));
    const int cur_nc = nc, cur_oy0 = oy0;
    const bool nxt = u + step < units;
    if (nxt) unit_of(u + step);
    dw_fetch(x + (size_t)nc * g.H * g.W, g.H, g.W, oy0 * ST - g.pt, d.IR, lane, rx, nxt);
    float wr[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) wr[t] = w[c * K * K + (FLIP ? K * K - 1 - t : t)];
    dw_wave_sync();
    const int oy = cur_oy0 + ro;
    const bool live = ro < d.RO && oy < g.P;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      const float *base = lds + (ro * ST) * d.WP + DW_PADL + ox0 * ST - g.pl;
#pragma unroll
      for (int a = 0; a < K; ++a) {
        float v[NV];
        dw_row<NV, OFF>(base + a * d.WP, v);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int b = 0; b < K; ++b) o[q] = __builtin_fmaf(wr[a * K + b], v[q * ST + b], o[q]);
      }
      st4(y + ((size_t)cur_nc * g.P + oy) * g.Q + ox0, make_float4(o[0], o[1], o[2], o[3]));
    }
    if (BS) {  // BatchNorm partials (separate instantiation)
      float f1 = 0.f, f2 = 0.f;
      if (live) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float v = stored<dw_to<B>>(o[q]);
          f1 += v;
          f2 = __builtin_fmaf(v, v, f2);
        }
      }
      const double s1 = dw_wave_sum((double)f1);
      const double s2 = dw_wave_sum((double)f2);
      if (lane == 0) {
        const int n = cur_nc / g.C, c = cur_nc - n * g.C;
        const size_t at = (((size_t)n * d.units_per_plane + cur_oy0 / d.RO) * g.C + c) * 2;
        stats[at] = s1;
        stats[at + 1] = s2;
      }
    }
    dw_wave_sync();  // LDS reuse
  }
}

template <int K, int ST, bool FLIP, int OFF, int V, bool BS = false, bool B = false>
__global__ void __launch_bounds__(256) k_dw_fwd_strip(const dw_ti<FLIP, B> *__restrict__ x,
                                                      const float *__restrict__ w, DwGeom g,
                                                      DwStrip d, int units, dw_to<B> *__restrict__ y,
                                                      DwIn tf, double *__restrict__ stats) {
  dw_fwd_strip_body<K, ST, FLIP, OFF, V, BS, B>(x, w, g, d, units, y, tf, stats, blockIdx.x,
                                                gridDim.x);
}

// stride-2 data gradient over strip units: a wave owns RO = 64/(W/4) rows of dx of one plane,
// each lane 4 adjacent dx pixels; the gy rows those rows read are staged in LDS.  For dx
// pixel ix only taps b with (ix + pl - b) even contribute; ix0 is a multiple of 4, so the
// parity of (u + pl - b) is compile-time given PLP = pl & 1.
// The block body for block blk (k_dw_dgrad_s2_strip, and the data-gradient half of
// k_dw_bwd_pair_s2), over the kernel's dynamic LDS.
template <int K, int PLP, bool B = false>
__device__ __forceinline__ void dw_dgrad_s2_body(const dw_to<B> *__restrict__ gy,
                                                 const float *__restrict__ w, DwGeom g, int RO,
                                                 int GR, int WPg, int units_per_plane, int units,
                                                 dw_to<B> *__restrict__ dx, int blk) {
  extern __shared__ float dw_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: SGPR descriptors
  const int unit = blk * 4 + wave;
  float *lds = dw_lds + wave * GR * WPg;
  const bool active = unit < units;
  int nc = 0, iy0 = 0, oyA = 0;
  if (active) {
    nc = unit / units_per_plane;
    iy0 = (unit - nc * units_per_plane) * RO;
    oyA = (iy0 + g.pt - (K - 1)) >> 1;  // floor division by 2
    dw_stage(gy + (size_t)nc * g.P * g.Q, g.P, g.Q, oyA, GR, WPg, lds, lane);
  }
  dw_wave_sync();
  if (!active) return;
  const int c = nc % g.C;
  float wr[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) wr[t] = w[c * K * K + t];
  const int WL = g.W >> 2;
  const int r = lane / WL, ix0 = 4 * (lane - r * WL);
  const int iy = iy0 + r;
  if (r >= RO || iy >= g.H) return;
  const int xoff = (ix0 >> 1) + ((g.pl - PLP) >> 1) + DW_PADL;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < K; ++a) {
    const int ny = iy + g.pt - a;
    if (ny & 1) continue;
    const float *row = lds + ((ny >> 1) - oyA) * WPg + xoff;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int b = 0; b < K; ++b)
        if (((u + PLP - b) & 1) == 0) o[u] = __builtin_fmaf(wr[a * K + b], row[(u + PLP - b) >> 1], o[u]);
  }
  st4(dx + ((size_t)nc * g.H + iy) * g.W + ix0, make_float4(o[0], o[1], o[2], o[3]));
}

template <int K, int PLP, bool B = false>
__global__ void __launch_bounds__(256) k_dw_dgrad_s2_strip(const dw_to<B> *__restrict__ gy,
                                                           const float *__restrict__ w, DwGeom g,
                                                           int RO, int GR, int WPg,
                                                           int units_per_plane, int units,
                                                           dw_to<B> *__restrict__ dx) {
  dw_dgrad_s2_body<K, PLP, B>(gy, w, g, RO, GR, WPg, units_per_plane, units, dx, blockIdx.x);
}

// weight gradient partials over strip units: grid (C, splits); the block's waves walk the
// channel's units (n, strip) of its slice; per lane K*K register accumulators, fixed-order
// wave + block reduction.
// The block body for channel c, split sp (k_dw_wgrad_strip, and the weight-gradient half of
// k_dw_bwd_pair), over the kernel's dynamic LDS.
template <int K, int ST, int OFF, int V, bool B = false>
__device__ __forceinline__ void dw_wgrad_strip_body(const dw_to<B> *__restrict__ gy,
                                                    const float *__restrict__ x, DwGeom g,
                                                    DwStrip d, int splits, DwPart part, DwIn tf,
                                                    int c, int sp) {
  extern __shared__ float dw_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: SGPR descriptors
  float *lds = dw_lds + wave * d.IR * d.WP;
  const int cunits = g.N * d.units_per_plane;  // units of this channel
  const int per = (cunits + splits - 1) / splits;
  const int beg = sp * per, end = min(cunits, beg + per);
  const int QL = g.Q >> 2;
  const int ro = lane / QL, ox0 = 4 * (lane - ro * QL);
  constexpr int NV = 3 * ST + K;
  float acc[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) acc[t] = 0.f;
  // Software-pipelined over the wave's units (u0 + wave, u0 + wave + 4, ...): the next unit's
  // input rows and gy row are loaded into registers before the current unit's FMAs, so the
  // load latency overlaps compute (the wave used to stage, wait, compute, one unit at a time:
  // 1.2-2.1 TB/s).  Up to DW_MAXV float4 per lane per unit (host-checked).
  auto unit_of = [&](int un, int &n, int &oy0) {
    n = un / d.units_per_plane;
    oy0 = (un - n * d.units_per_plane) * d.RO;
  };
  float4 rx[V];
  float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
  constexpr int GB = sizeof(dw_to<B>);  // bytes per gy element
  const __amdgpu_buffer_rsrc_t rgy = rsrc(gy, (long long)GB * g.N * g.C * g.P * g.Q);
  int n = 0, oy0 = 0;
  bool active = beg + wave < end;
  if (active) unit_of(beg + wave, n, oy0);
  auto fetch = [&](bool act, int nn, int yy0) {
    dw_fetch(x + ((size_t)nn * g.C + c) * g.H * g.W, g.H, g.W, yy0 * ST - g.pt, d.IR, lane, rx, act);
    const int oy = yy0 + ro;
    const bool ok = act && ro < d.RO && oy < g.P;
    gq = bload4t(rgy, ok ? (((nn * g.C + c) * g.P + oy) * g.Q + ox0) * GB : OOR, gy);
  };
  const DwT tfc = dw_t(tf, c);  // the block's channel: read once
  fetch(active, n, oy0);
  for (int u0 = beg; u0 < end; u0 += 4) {
    dw_put(rx, g.H, g.W, oy0 * ST - g.pt, d.IR, d.WP, lds, lane, tfc);
    const float gv[4] = {gq.x, gq.y, gq.z, gq.w};
    const bool cur_active = active;
    const int cur_oy0 = oy0;
    // next unit of this wave: its loads fly while this unit computes
    const bool nxt = u0 + 4 + wave < end;
    int nn = 0, noy0 = 0;
    if (nxt) unit_of(u0 + 4 + wave, nn, noy0);
    fetch(nxt, nn, noy0);
    active = nxt;
    n = nn;
    oy0 = noy0;
    dw_wave_sync();
    const int oy = cur_oy0 + ro;
    if (cur_active && ro < d.RO && oy < g.P) {
      const float *base = lds + (ro * ST) * d.WP + DW_PADL + ox0 * ST - g.pl;
#pragma unroll
      for (int a = 0; a < K; ++a) {
        float v[NV];
        dw_row<NV, OFF>(base + a * d.WP, v);
#pragma unroll
        for (int b = 0; b < K; ++b)
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[a * K + b] = __builtin_fmaf(gv[u], v[u * ST + b], acc[a * K + b]);
      }
    }
    dw_wave_sync();  // LDS reuse
  }
  __shared__ float red[4][K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) {
    const float v = wave_sum(acc[t]);
    if (lane == 0) red[wave][t] = v;
  }
  __syncthreads();
  const int t = threadIdx.x < K * K ? threadIdx.x : 0;
  // the last-arriver flag reuses red[0][0] (read above, before dw_wgrad_out's first barrier):
  // a static __shared__ int would leave the kernel's static LDS at 4 mod 16 bytes and shift the
  // strip kernels' dynamic LDS base off 16-B alignment (their b128 window reads then replay:
  // 1.5 - 2x slower; cdna_hip_programming.md Guideline 17)
  dw_wgrad_out<K * K>(part, c, sp, splits, (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]),
                      reinterpret_cast<int *>(&red[0][0]));
}

template <int K, int ST, int OFF, int V, bool B = false>
__global__ void __launch_bounds__(256) k_dw_wgrad_strip(const dw_to<B> *__restrict__ gy,
                                                        const float *__restrict__ x, DwGeom g,
                                                        DwStrip d, int splits,
                                                        DwPart part, DwIn tf) {
  dw_wgrad_strip_body<K, ST, OFF, V, B>(gy, x, g, d, splits, part, tf, blockIdx.x, blockIdx.y);
}

// A stride-1 depthwise layer's data gradient (the flipped-filter strip forward over gy, gt /
// dt its geometry) and weight gradient (strip partials, g / d) in one grid: block c + C * sp
// (< nw = C * splits) the weight gradient of channel c, split sp, the nd blocks after them
// walk the data-gradient units grid-stride.  The weight-gradient blocks go first: each walks
// a channel's units of its split (tens per wave) and ends in a block reduction, the long
// poles of the launch; queued behind the data-gradient blocks they ran last and serial
// (67.5 us against 52 us for the weight gradient alone).  One launch instead of two on
// forked streams (e2ep_dwconv_bwd): in a replayed graph the fork / join idles the GPU ~17 us
// per layer.  Dynamic LDS: the larger of the two halves' per-wave row buffers.
template <int K, int OFF, int VD, int VW, bool B = false>
__global__ void __launch_bounds__(256) k_dw_bwd_pair(const dw_to<B> *__restrict__ gy,
                                                     const float *__restrict__ w, DwGeom gt,
                                                     DwStrip dt, int units, dw_to<B> *__restrict__ dx,
                                                     int nd, const float *__restrict__ x, DwGeom g,
                                                     DwStrip d, int splits, DwPart part, DwIn tf) {
  const int b = blockIdx.x, nw = g.C * splits;
  if (b < nw) {
    dw_wgrad_strip_body<K, 1, OFF, VW, B>(gy, x, g, d, splits, part, tf, b % g.C, b / g.C);
  } else {
    dw_fwd_strip_body<K, 1, true, OFF, VD, false, B>(gy, w, gt, dt, units, dx,
                                                     DwIn{nullptr, nullptr, 0}, nullptr, b - nw, nd);
  }
}

// The stride-2 form of k_dw_bwd_pair: weight-gradient blocks first (channel c, split sp), then
// the k_dw_dgrad_s2_strip blocks (one unit per wave).
template <int K, int PLP, int OFF, int VW, bool B = false>
__global__ void __launch_bounds__(256) k_dw_bwd_pair_s2(const dw_to<B> *__restrict__ gy,
                                                        const float *__restrict__ w, int RO, int GR,
                                                        int WPg, int upp2, int units2,
                                                        dw_to<B> *__restrict__ dx,
                                                        const float *__restrict__ x, DwGeom g,
                                                        DwStrip d, int splits, DwPart part, DwIn tf) {
  const int b = blockIdx.x, nw = g.C * splits;
  if (b < nw)
    dw_wgrad_strip_body<K, 2, OFF, VW, B>(gy, x, g, d, splits, part, tf, b % g.C, b / g.C);
  else
    dw_dgrad_s2_body<K, PLP, B>(gy, w, g, RO, GR, WPg, upp2, units2, dx, b - nw);
}

static DwGeom dw_geom(const int *d) {
  DwGeom g;
  g.N = d[0]; g.C = d[1]; g.H = d[2]; g.W = d[3]; g.K = d[4]; g.P = d[5]; g.Q = d[6];
  g.st = d[7]; g.pt = d[8]; g.pl = d[9];
  return g;
}

// ---- launch plan -------------------------------------------------------------------------
// dw_plan() is the only place that says which kernel runs for a geometry; the launchers, the
// statistics / pair / storage / workspace queries and the paired backward all read its answer.

// grid of the forward strip kernel: one unit per wave up to e2ep_tune key 24 blocks
static int dw_fwd_blocks(int units) { return std::min(cdiv(units, 4), g_tune[TUNE_DW_FWD_BLOCKS]); }
// the strip kernels' LDS row-read variant: dw_row's OFF for left pad pl, or -1 (scalar reads,
// e2ep_tune key 23 = 1)
static int dw_off(int pl) { return g_tune[TUNE_DW_VEC] == 1 ? -1 : ((-pl) & 3); }

// One geometry on k_dw_fwd_strip / k_dw_wgrad_strip: the unit shape, the forward grid
// (`blocks`), the dynamic LDS, the row-read variant `off` as the kernels' compile-time OFF and
// the staging registers V = 2 float4 per lane where a unit's IR * W / 4 float4 allow (the
// scalar-read variant, an A/B switch, always takes DW_MAXV).
struct DwRoute {
  bool ok;
  DwGeom g;
  DwStrip d;
  int units, blocks, off, v;
  size_t lds;
};

// The strip gate.  Shape: Q % 4 == 0 and Q <= 256 (a unit is 64 lanes x 4 outputs), W % 4 == 0
// (float4 staging), an instantiated (K, stride), and a unit's rows within the unrolled
// staging's reach (IR * W / 4 <= 64 * DW_MAXV float4).
// Halo: a staged row holds WP = W + 2 * DW_PADL floats, [0, DW_PADL) and [DW_PADL + W, WP) zero.
// The lane at output column ox0 (0, 4, .., Q - 4) reads its window row from
//   base = DW_PADL + ox0 * ST - pl   (dw_fwd_strip_body / dw_wgrad_strip_body),
// NV = 3 * ST + K floats.  The scalar reads (OFF = -1) touch [base, base + NV): inside [0, WP)
// for every lane iff
//   pl <= DW_PADL   and   DW_PADL + (Q - 4) * ST - pl + 3 * ST + K <= WP,
// the second being "the right pad the output width implies, (Q - 1) * ST + K - pl - W, is at
// most DW_PADL".  The vector reads (dw_row, OFF = -pl mod 4) touch [base - OFF,
// base - OFF + 4 * ceil((OFF + NV) / 4)): base - OFF is base rounded down to a multiple of 4
// (DW_PADL, ox0 * ST and pl + OFF are multiples of 4) and the end is base + NV rounded up to
// one; 0 and WP are multiples of 4, so the same two inequalities bound the vector reads.  TF
// "same" pads (at most 2 left, 3 right) always satisfy them; a larger asymmetric pad takes the
// generic kernels.
static DwRoute dw_route(const DwGeom &g) {
  DwRoute r{};
  r.g = g;
  if (!(g.Q % 4 == 0 && g.Q <= 256 && g.W % 4 == 0 && (g.K == 3 || g.K == 5) &&
        (g.st == 1 || g.st == 2)))
    return r;
  r.d = dw_strip(g.K, g.st, g.W, g.P, g.Q);
  const int nv = r.d.IR * (g.W / 4);  // float4 of a unit's rows
  if (nv > 64 * DW_MAXV) return r;
  if (g.pl > DW_PADL || DW_PADL + (g.Q - 4) * g.st - g.pl + 3 * g.st + g.K > r.d.WP) return r;
  r.ok = true;
  r.units = g.N * g.C * r.d.units_per_plane;
  r.blocks = dw_fwd_blocks(r.units);
  r.off = dw_off(g.pl);
  r.v = r.off >= 0 && cdiv(nv, 64) <= 2 ? 2 : DW_MAXV;
  r.lds = 4 * r.d.IR * r.d.WP * sizeof(float);
  return r;
}

// stride 1: dx = gy (P x Q) correlated with the flipped filter, pads K-1-pad, output H x W
static DwRoute dw_route_flipped(const DwGeom &g) {
  DwGeom t = g;
  t.H = g.P; t.W = g.Q; t.P = g.H; t.Q = g.W;
  t.pt = g.K - 1 - g.pt; t.pl = g.K - 1 - g.pl;
  if (g.st != 1 || t.pt < 0 || t.pl < 0) return DwRoute{};
  return dw_route(t);
}

// The stride-2 data-gradient strip plan (RO dx rows per unit, GR gy rows staged, one unit per
// wave); false where the data gradient runs the generic kernel.
// Halo: a staged gy row holds WPg = Q + 2 * DW_PADL floats.  The lane at dx column ix0 (0, 4,
// .., W - 4) reads column DW_PADL + ix0 / 2 + (pl - PLP) / 2 + (u + PLP - b) / 2 for u < 4 and
// the taps b < K with u + PLP - b even (dw_dgrad_s2_body): lowest at ix0 = 0, u = 0 and the
// largest such b (K - 1 - PLP), highest at ix0 = W - 4, u = 3 and the smallest (1 - PLP).
struct DwS2 {
  int RO, GR, WPg, upp, units, blocks;
  size_t lds;
};
static bool dw_s2_plan(const DwGeom &g, DwS2 &p) {
  if (!(g.st == 2 && g.W % 4 == 0 && g.W <= 256 && g.Q % 4 == 0 && (g.K == 3 || g.K == 5) &&
        g.pl <= 2 && g.pt <= 2))
    return false;
  p.RO = 64 / (g.W / 4);
  p.GR = ((p.RO - 1 + g.pt) >> 1) - ((g.pt - (g.K - 1)) >> 1) + 2;
  if (p.GR * (g.Q / 4) > 64 * DW_MAXV) return false;
  p.WPg = g.Q + 2 * DW_PADL;
  const int plp = g.pl & 1, x0 = DW_PADL + ((g.pl - plp) >> 1);
  if (x0 - ((g.K - 1 - plp) >> 1) < 0 || x0 + (g.W - 4) / 2 + 1 + plp >= p.WPg) return false;
  p.upp = (g.H + p.RO - 1) / p.RO;
  p.units = g.N * g.C * p.upp;
  p.blocks = cdiv(p.units, 4);
  p.lds = 4 * p.GR * p.WPg * sizeof(float);
  return true;
}

// Not for stride-2 data gradients of more than DW_S2_PAIR_UNITS units: the 128 x 128-map layer
// (294 912 units) ran 220 us paired against ~183 us as two forked launches, while the 43 008-
// and 98 304-unit layers ran 37 / 87 us paired against ~44 / ~86 us forked
// (step_sequence_fp32_final.txt against _r4z.txt).
constexpr int DW_S2_PAIR_UNITS = 131072;

enum DwKind { DW_GENERIC, DW_STRIP, DW_STRIP_S2 };
enum DwPair { DW_PAIR_NONE, DW_PAIR_S1, DW_PAIR_S2 };
struct DwPlan {
  bool valid;        // N, C, P, Q, stride > 0; nothing below is set otherwise
  DwGeom g;
  int fwd, wgrad;    // DW_STRIP: k_dw_fwd_strip / k_dw_wgrad_strip on route s; else k_dw_fwd / k_dw_wgrad
  int dgrad;         // DW_STRIP: k_dw_fwd_strip<FLIP> on route t (stride 1); DW_STRIP_S2:
                     // k_dw_dgrad_s2_strip on s2; else k_dw_dgrad
  DwRoute s, t;
  DwS2 s2;
  int stats_tiles;   // units per channel: the forward's BatchNorm partial sums, 0 = not taken
  int splits;        // weight-gradient slabs
  size_t workspace;  // bytes of the slabs
  int pair;          // e2ep_dwconv_bwd: both gradients in k_dw_bwd_pair (S1) / k_dw_bwd_pair_s2 (S2)
  int fwd_io, dgrad_io, wgrad_io;  // E2EP_IO_* storage mask each direction accepts besides 0
  bool bf16_ok;      // every kernel of the layer, and the BatchNorms beside it, take bf16 storage
};

// Gates in order.  Forward and weight gradient: the strip kernels where dw_route(g), else the
// generic ones.  Data gradient: the flipped strip forward (stride 1, dw_route of the flipped
// geometry), the stride-2 strip kernel (dw_s2_plan), else the generic one.  Paired backward:
// both halves on strip kernels with vector row reads at an instantiated combination:
// stride 1 with one OFF for both halves (symmetric padding, K = 3 pad 1 -> 3, K = 5 pad 2 -> 2);
// stride 2 at K = 3 pad_left 0 / 1, K = 5 pad_left 1 / 2, up to DW_S2_PAIR_UNITS units.
static DwPlan dw_plan(const DwGeom &g) {
  DwPlan p{};
  p.g = g;
  p.valid = g.N > 0 && g.C > 0 && g.P > 0 && g.Q > 0 && g.st > 0;
  if (!p.valid) return p;
  p.s = dw_route(g);
  p.t = dw_route_flipped(g);
  if (p.s.ok) {
    p.fwd = p.wgrad = DW_STRIP;
    p.stats_tiles = g.N * p.s.d.units_per_plane;
    p.fwd_io = E2EP_IO_DX_BF16;
    p.wgrad_io = E2EP_IO_DY_BF16;
  }
  p.dgrad = p.t.ok ? DW_STRIP : dw_s2_plan(g, p.s2) ? DW_STRIP_S2 : DW_GENERIC;
  if (p.dgrad != DW_GENERIC) p.dgrad_io = E2EP_IO_DY_BF16 | E2EP_IO_DX_BF16;
  // slabs: e2ep_tune key 3 workgroups (generic kernel: 1024) over the C channels, each split
  // of >= 8 units, 2 per wave (generic: >= 2048 pixels); 1 .. 128
  const bool ws = p.wgrad == DW_STRIP;
  const long long want = cdiv(ws ? g_tune[TUNE_DW_WGRAD_TARGET] : 1024, g.C);
  const long long cap = ws ? (p.stats_tiles + 7) / 8 : (long long)g.N * g.P * g.Q / 2048;
  p.splits = (int)std::max(1LL, std::min({want, cap, 128LL}));
  p.workspace = (size_t)g.C * p.splits * g.K * g.K * sizeof(float);
  if (p.wgrad == DW_STRIP && p.s.off >= 0) {
    if (p.dgrad == DW_STRIP && p.t.off == p.s.off && p.s.off == (g.K == 3 ? 3 : 2))
      p.pair = DW_PAIR_S1;
    else if (p.dgrad == DW_STRIP_S2 && p.s2.units <= DW_S2_PAIR_UNITS &&
             (g.K == 3 ? g.pl == 0 || g.pl == 1 : g.pl == 1 || g.pl == 2))
      p.pair = DW_PAIR_S2;
  }
  p.bf16_ok = p.fwd == DW_STRIP && p.dgrad != DW_GENERIC && (g.H * g.W) % 4 == 0 &&
              (g.P * g.Q) % 4 == 0;
  return p;
}

// ---- template dispatch: f is a generic lambda taking integral constants (common.h IntC) -----
// f(K, ST) for the instantiated filters and strides; E2EP_ERANGE for any other
template <class F> static int with_k_st(const DwGeom &g, F f) {
  if (g.K == 3 && g.st == 1) f(IntC<3>(), IntC<1>());
  else if (g.K == 3 && g.st == 2) f(IntC<3>(), IntC<2>());
  else if (g.K == 5 && g.st == 1) f(IntC<5>(), IntC<1>());
  else if (g.K == 5 && g.st == 2) f(IntC<5>(), IntC<2>());
  else {
    set_error("depthwise conv: kernel %d / stride %d unsupported (k 3|5, s 1|2)", g.K, g.st);
    return E2EP_ERANGE;
  }
  return 0;
}
// f(K), K = 3 or 5 (the strip routes have no other)
template <class F> static void with_k(int K, F f) {
  if (K == 3) f(IntC<3>());
  else f(IntC<5>());
}
// f(0 / 1) for a two-way choice (bf16 storage, statistics, pad parity)
template <class F> static void with_flag(bool on, F f) {
  if (on) f(IntC<1>());
  else f(IntC<0>());
}
// f(V), V = 2 or DW_MAXV staging registers
template <class F> static void with_v(int v, F f) {
  if (v == 2) f(IntC<2>());
  else f(IntC<DW_MAXV>());
}
// f(OFF, V) of a DwRoute: OFF = -1 exists only with V = DW_MAXV
template <class F> static void with_off_v(const DwRoute &r, F f) {
  if (r.off < 0) return f(IntC<-1>(), IntC<DW_MAXV>());
  with_v(r.v, [&](auto v) {
    if (r.off == 0) f(IntC<0>(), v);
    else if (r.off == 1) f(IntC<1>(), v);
    else if (r.off == 2) f(IntC<2>(), v);
    else f(IntC<3>(), v);
  });
}

// k_dw_fwd_strip on route r: the forward (statistics where `stats`), or with FLIP the
// stride-1 data gradient, which takes none (no <FLIP, BS> kernel exists)
template <bool FLIP>
static void dw_launch_fwd_strip(const DwRoute &r, bool b16, const void *x, const float *w, void *y,
                                DwIn tf, double *stats, hipStream_t s) {
  with_k_st(r.g, [&](auto k, auto st) {
    with_off_v(r, [&](auto off, auto v) {
      with_flag(b16, [&](auto b) {
        with_flag(stats != nullptr, [&](auto bs) {
          constexpr int K = decltype(k)::value, ST = decltype(st)::value;
          constexpr bool B = decltype(b)::value != 0, BS = decltype(bs)::value != 0;
          if constexpr (!FLIP || (ST == 1 && !BS))
            hipLaunchKernelGGL((k_dw_fwd_strip<K, ST, FLIP, decltype(off)::value, decltype(v)::value, BS, B>),
                               dim3(r.blocks), dim3(256), r.lds, s,
                               static_cast<const dw_ti<FLIP, B> *>(x), w, r.g, r.d, r.units,
                               static_cast<dw_to<B> *>(y), tf, stats);
        });
      });
    });
  });
}

static void dw_launch_dgrad_s2(const DwPlan &p, bool b16, const void *gy, const float *w, void *dx,
                               hipStream_t s) {
  const DwS2 &q = p.s2;
  with_k(p.g.K, [&](auto k) {
    with_flag(p.g.pl & 1, [&](auto plp) {
      with_flag(b16, [&](auto b) {
        constexpr bool B = decltype(b)::value != 0;
        hipLaunchKernelGGL((k_dw_dgrad_s2_strip<decltype(k)::value, decltype(plp)::value, B>),
                           dim3(q.blocks), dim3(256), q.lds, s, static_cast<const dw_to<B> *>(gy), w,
                           p.g, q.RO, q.GR, q.WPg, q.upp, q.units, static_cast<dw_to<B> *>(dx));
      });
    });
  });
}

static void dw_launch_wgrad_strip(const DwPlan &p, bool b16, const void *gy, const float *x,
                                  DwPart part, DwIn tf, hipStream_t s) {
  const DwRoute &r = p.s;
  with_k_st(r.g, [&](auto k, auto st) {
    with_off_v(r, [&](auto off, auto v) {
      with_flag(b16, [&](auto b) {
        constexpr bool B = decltype(b)::value != 0;
        hipLaunchKernelGGL((k_dw_wgrad_strip<decltype(k)::value, decltype(st)::value,
                                             decltype(off)::value, decltype(v)::value, B>),
                           dim3(r.g.C, p.splits), dim3(256), r.lds, s,
                           static_cast<const dw_to<B> *>(gy), x, r.g, r.d, p.splits, part, tf);
      });
    });
  });
}

// k_dw_bwd_pair: the weight-gradient blocks, then the data-gradient blocks of route t
static void dw_launch_pair_s1(const DwPlan &p, bool b16, const void *gy, const float *x,
                              const float *w, void *dx, DwPart part, DwIn tf, hipStream_t s) {
  const DwRoute &r = p.s, &t = p.t;
  with_k(p.g.K, [&](auto k) {
    with_v(t.v, [&](auto vd) {
      with_v(r.v, [&](auto vw) {
        with_flag(b16, [&](auto b) {
          constexpr int K = decltype(k)::value, OFF = K == 3 ? 3 : 2;
          constexpr bool B = decltype(b)::value != 0;
          hipLaunchKernelGGL((k_dw_bwd_pair<K, OFF, decltype(vd)::value, decltype(vw)::value, B>),
                             dim3(t.blocks + r.g.C * p.splits), dim3(256), std::max(t.lds, r.lds), s,
                             static_cast<const dw_to<B> *>(gy), w, t.g, t.d, t.units,
                             static_cast<dw_to<B> *>(dx), t.blocks, x, r.g, r.d, p.splits, part, tf);
        });
      });
    });
  });
}

// k_dw_bwd_pair_s2: PLP = pad_left & 1, OFF = -pad_left mod 4 (dw_off) of the four instantiated
// (K, pad_left): K = 3 pad 0 / 1 -> OFF 0 / 3, K = 5 pad 1 / 2 -> OFF 3 / 2
static void dw_launch_pair_s2(const DwPlan &p, bool b16, const void *gy, const float *x,
                              const float *w, void *dx, DwPart part, DwIn tf, hipStream_t s) {
  const DwRoute &r = p.s;
  const DwS2 &q = p.s2;
  with_k(p.g.K, [&](auto k) {
    with_flag(p.g.pl & 1, [&](auto plp) {
      with_v(r.v, [&](auto vw) {
        with_flag(b16, [&](auto b) {
          constexpr int K = decltype(k)::value, PLP = decltype(plp)::value;
          constexpr int OFF = PLP ? 3 : K == 3 ? 0 : 2;
          constexpr bool B = decltype(b)::value != 0;
          hipLaunchKernelGGL((k_dw_bwd_pair_s2<K, PLP, OFF, decltype(vw)::value, B>),
                             dim3(r.g.C * p.splits + q.blocks), dim3(256), std::max(q.lds, r.lds), s,
                             static_cast<const dw_to<B> *>(gy), w, q.RO, q.GR, q.WPg, q.upp, q.units,
                             static_cast<dw_to<B> *>(dx), x, r.g, r.d, p.splits, part, tf);
        });
      });
    });
  });
}

// one split: the slab is the gradient; several: in-launch fold (e2ep_tune key 28 = 2) or
// k_dw_wgrad_finalize after the launch (dw_finalize)
static DwPart dw_part(const DwPlan &p, void *workspace, float *dw, hipStream_t s) {
  return DwPart{static_cast<float *>(workspace), dw,
                (p.splits > 1 && g_tune[TUNE_SPLITK_FOLD] == 2) ? handoff_slots(p.g.C, s) : nullptr};
}
static void dw_finalize(const DwPlan &p, const DwPart &part, hipStream_t s) {
  const int KK = p.g.K * p.g.K;
  if (p.splits > 1 && !part.cnt)
    hipLaunchKernelGGL(k_dw_wgrad_finalize, dim3(cdiv(p.g.C * KK, 256)), dim3(256), 0, s, part.part,
                       p.g.C, KK, p.splits, part.dw);
}

// What the launch entry points require, in one place (0, or the status to hand back): a
// geometry; a storage mask that is 0 or the one (io_ok) the planned kernel takes; an input
// transform with both vectors or neither; where need_ws, the weight gradient's slabs.
static int dw_check(const char *fn, const DwPlan &p, int io, int io_ok,
                    DwIn tf = DwIn{nullptr, nullptr, 0}, bool need_ws = false,
                    const void *workspace = nullptr, size_t workspace_bytes = 0) {
  E2EP_REQUIRE(p.valid, E2EP_EINVAL, "%s: bad geometry", fn);
  E2EP_REQUIRE(io == 0 || io == io_ok, E2EP_EINVAL, "%s: storage mask %d not supported (0, or %d "
               "(E2EP_IO_*) where the strip kernels run)", fn, io, io_ok);
  E2EP_REQUIRE(!tf.sc == !tf.sh && tf.act >= 0 && tf.act <= 2, E2EP_EINVAL,
               "%s: in_scale / in_shift both or neither, in_act 0..2", fn);
  E2EP_REQUIRE(!need_ws || (workspace && workspace_bytes >= p.workspace), E2EP_EINVAL,
               "%s: workspace %zu bytes < %zu (e2ep_dwconv_wgrad_workspace)", fn, workspace_bytes,
               p.workspace);
  return 0;
}

}  // namespace e2ep

using namespace e2ep;

extern "C" {

// dims[10] = {N, C, H, W, K, P, Q, stride, pad_top, pad_left}
int e2ep_dwconv_fwd_stats_tiles(const int *dims) { return dw_plan(dw_geom(dims)).stats_tiles; }

int e2ep_dwconv_bwd_pair_ok(const int *dims) {
  return dw_plan(dw_geom(dims)).pair != DW_PAIR_NONE ? 1 : 0;
}

int e2ep_dwconv_bf16_ok(const int *dims) { return dw_plan(dw_geom(dims)).bf16_ok ? 1 : 0; }

size_t e2ep_dwconv_wgrad_workspace(const int *dims) { return dw_plan(dw_geom(dims)).workspace; }

int e2ep_dwconv_fwd(const float *x, const float *w, const int *dims, const float *in_scale,
                    const float *in_shift, int in_act, float *y, void *stream) {
  return e2ep_dwconv_fwd_stats(x, w, dims, in_scale, in_shift, in_act, y, nullptr, 0, stream, 0);
}

int e2ep_dwconv_fwd_stats(const float *x, const float *w, const int *dims, const float *in_scale,
                          const float *in_shift, int in_act, void *y, double *stats,
                          size_t stats_bytes, void *stream, int io) {
  const char *fn = "e2ep_dwconv_fwd_stats";
  const DwPlan p = dw_plan(dw_geom(dims));
  const DwGeom &g = p.g;
  const DwIn tf{in_scale, in_shift, in_act};
  if (int e = dw_check(fn, p, io, p.fwd_io, tf)) return e;
  if (stats) {
    E2EP_REQUIRE(p.stats_tiles > 0, E2EP_EINVAL, "%s: this geometry's kernel takes no statistics", fn);
    const size_t need = (size_t)g.C * p.stats_tiles * 2 * sizeof(double);
    E2EP_REQUIRE(stats_bytes >= need, E2EP_EINVAL, "%s: stats %zu bytes < %zu (C x tiles x 2 doubles)",
                 fn, stats_bytes, need);
  }
  hipStream_t s = as_stream(stream);
  if (p.fwd == DW_STRIP) {
    dw_launch_fwd_strip<false>(p.s, io != 0, x, w, y, tf, stats, s);
    return launch_status(fn);
  }
  E2EP_REQUIRE(g.N * g.C <= 65535, E2EP_ERANGE, "%s: N*C > 65535", fn);
  const int e = with_k_st(g, [&](auto k, auto st) {
    hipLaunchKernelGGL((k_dw_fwd<decltype(k)::value, decltype(st)::value>),
                       dim3(cdiv(g.P * g.Q, 256), g.N * g.C), dim3(256), 0, s, x, w, g,
                       static_cast<float *>(y), in_scale, in_shift, in_act);
  });
  return e ? e : launch_status(fn);
}

int e2ep_dwconv_dgrad(const void *gy, const float *w, const int *dims, void *dx, void *stream,
                      int io) {
  const char *fn = "e2ep_dwconv_dgrad";
  const DwPlan p = dw_plan(dw_geom(dims));
  const DwGeom &g = p.g;
  if (int e = dw_check(fn, p, io, p.dgrad_io)) return e;
  hipStream_t s = as_stream(stream);
  if (p.dgrad == DW_STRIP) {
    dw_launch_fwd_strip<true>(p.t, io != 0, gy, w, dx, DwIn{nullptr, nullptr, 0}, nullptr, s);
    return launch_status(fn);
  }
  if (p.dgrad == DW_STRIP_S2) {
    dw_launch_dgrad_s2(p, io != 0, gy, w, dx, s);
    return launch_status(fn);
  }
  E2EP_REQUIRE(g.N * g.C <= 65535, E2EP_ERANGE, "%s: N*C > 65535", fn);
  const int e = with_k_st(g, [&](auto k, auto st) {
    hipLaunchKernelGGL((k_dw_dgrad<decltype(k)::value, decltype(st)::value>),
                       dim3(cdiv(g.H * g.W, 256), g.N * g.C), dim3(256), 0, s,
                       static_cast<const float *>(gy), w, g, static_cast<float *>(dx));
  });
  return e ? e : launch_status(fn);
}

int e2ep_dwconv_wgrad(const void *gy, const float *x, const int *dims, const float *in_scale,
                      const float *in_shift, int in_act, void *workspace, size_t workspace_bytes,
                      float *dw, void *stream, int io) {
  const char *fn = "e2ep_dwconv_wgrad";
  const DwPlan p = dw_plan(dw_geom(dims));
  const DwGeom &g = p.g;
  const DwIn tf{in_scale, in_shift, in_act};
  if (int e = dw_check(fn, p, io, p.wgrad_io, tf, true, workspace, workspace_bytes)) return e;
  hipStream_t s = as_stream(stream);
  const DwPart part = dw_part(p, workspace, dw, s);
  if (p.wgrad == DW_STRIP) {
    dw_launch_wgrad_strip(p, io != 0, gy, x, part, tf, s);
  } else {
    const int e = with_k_st(g, [&](auto k, auto st) {
      hipLaunchKernelGGL((k_dw_wgrad<decltype(k)::value, decltype(st)::value>), dim3(g.C, p.splits),
                         dim3(256), 0, s, static_cast<const float *>(gy), x, g, p.splits, part,
                         in_scale, in_shift, in_act);
    });
    if (e) return e;
  }
  dw_finalize(p, part, s);
  return launch_status(fn);
}

int e2ep_dwconv_bwd(const void *gy, const float *x, const float *w, const int *dims,
                    const float *in_scale, const float *in_shift, int in_act, void *dx,
                    void *workspace, size_t workspace_bytes, float *dw, void *stream, int io) {
  const char *fn = "e2ep_dwconv_bwd";
  const DwPlan p = dw_plan(dw_geom(dims));
  const DwIn tf{in_scale, in_shift, in_act};
  if (int e = dw_check(fn, p, io, p.dgrad_io, tf, true, workspace, workspace_bytes)) return e;
  E2EP_REQUIRE(p.pair != DW_PAIR_NONE, E2EP_EINVAL,
               "%s: no paired backward for this geometry (e2ep_dwconv_bwd_pair_ok returned 0)", fn);
  E2EP_REQUIRE(gy && x && w && dx && dw, E2EP_EINVAL, "%s: null tensor", fn);
  hipStream_t s = as_stream(stream);
  const DwPart part = dw_part(p, workspace, dw, s);
  if (p.pair == DW_PAIR_S1) dw_launch_pair_s1(p, io != 0, gy, x, w, dx, part, tf, s);
  else dw_launch_pair_s2(p, io != 0, gy, x, w, dx, part, tf, s);
  dw_finalize(p, part, s);
  return launch_status(fn);
}

}  // extern "C"

