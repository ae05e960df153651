// Strided fp32 GEMM on MFMA for the transformer linears (nn.Linear forward and both
// backward GEMMs of model/feature_fusion.py:13-14,24-29,48-50 and model/control_predict.py:
// 18-24: d = 258 / 774 / 2048 at 2048 encoder rows and 112 decoder rows).
//
//   C[m][n] = sum_k A(m, k) * B(k, n)  (+ bias[n])  (+ Cadd[m][n])  (then ReLU if asked)
//   A(m, k) = AK ? A[m * lda + k] : A[k * lda + m]
//   B(k, n) = BKC ? B[n * ldb + k] : B[k * ldb + n]
//
// Forward y = x W^T + b is (AK, BKC); dX = dY W is (AK, !BKC); dW = dY^T X is (!AK, !BKC).
// Design (the k_conv_gemm2 scheme, CDNA4 fp32 MFMA v_mfma_f32_32x32x2_f32):
//  * block (64 TM) x (64 TN), 4 waves as 2 x 2, wave tile 32 TM x 32 TN (each A fragment
//    feeds TN MFMAs, each B fragment TM); K-step 32;
//  * LDS rows are k-contiguous ([row][32 + 4 pad]) whatever the global layout, so a lane's
//    16 fragment values are four ds_read_b128 (lane half h supplies k = 16h..16h+15 to the 16
//    MFMAs of a step — the sum over the 32 k is the same, its order fixed);
//  * global loads are raw buffer loads with out-of-range offsets for the M / N / K edges
//    (returns 0: no padding copies, K = 258 needs no special case); the next step's tile is
//    loaded into registers while the current one feeds the MFMAs;
//  * small grids split K (fixed-order reduction in k_gemm_reduce, so results are
//    deterministic run to run), large ones write C directly with the fused epilogue.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "gemm.h"
#include "handoff.h"

namespace e2ep {

typedef float g_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 g_bf16x8 __attribute__((ext_vector_type(8)));

// bload2 (8-B buffer load): common.h

// v & (ok ? ~0 : 0) as one v_and_b32 the compiler cannot turn back into a branch
__device__ __forceinline__ float kmask(float v, bool ok) {
  const unsigned m = ok ? 0xffffffffu : 0u;
  unsigned r;
  asm volatile("v_and_b32 %0, %1, %2" : "=v"(r) : "v"(__builtin_bit_cast(unsigned, v)), "v"(m));
  return __builtin_bit_cast(float, r);
}
constexpr int G_BK = 32;
constexpr int G_LDW = 36;  // LDS row stride in floats (32 k + 4 pad)

// OP: MFMA operand precision, 0 = fp32 (v_mfma_f32_32x32x2_f32, exact), 1 = bf16 (BASELINE
// C3: the fragments are rounded to bf16 when read from LDS, two v_mfma_f32_32x32x16_bf16 per
// 32-deep step, products and sums fp32; HBM tensors stay fp32)
// One GEMM problem of a launch: operands, epilogue inputs, its tile grid (gx column tiles x gy
// row tiles x gz K splits) and split-K fold state.
struct GemmArgs {
  const float *A;
  int lda;
  long long a_bytes;
  const float *B;
  int ldb;
  long long b_bytes;
  const float *bias;
  int bias_rows;
  const float *Cadd;
  int ldadd;
  float *C;
  long long c_bytes;
  int ldc;
  GemmCols cols;
  int M, N, K, kper, relu;
  float *rs, *part;
  unsigned int *cnt;
  int gx, gy, gz;
};

template <bool AK_, bool BKC_, int WM_, int TM_, int TN_, int AVEC_, int BVEC_, int OP_>
struct GemmCfg {
  static constexpr bool AK = AK_, BKC = BKC_;
  static constexpr int WM = WM_, TM = TM_, TN = TN_, AVEC = AVEC_, BVEC = BVEC_, OP = OP_;
  static constexpr int BM = 32 * TM * WM, BN = 32 * TN * (4 / WM);
  static constexpr int LDS_FLOATS = 2 * (BM + BN) * G_LDW;  // As[2][BM][G_LDW], Bs[2][BN][G_LDW]
};

// The block body of k_gemm for block (bx, by, bz) of problem g; `lds` holds CFG::LDS_FLOATS
// floats (16-B aligned) and s_last one int, both __shared__ of the calling kernel (so a kernel
// running two problems, k_gemm_pair, shares one LDS allocation between them).
template <class CFG>
__device__ __forceinline__ void gemm_block(const GemmArgs &g, int bx, int by, int bz, float *lds,
                                           int *s_last) {
  constexpr bool AK = CFG::AK, BKC = CFG::BKC;
  constexpr int WM = CFG::WM, TM = CFG::TM, TN = CFG::TN, AVEC = CFG::AVEC, BVEC = CFG::BVEC,
                OP = CFG::OP;
  const float *__restrict__ A = g.A;
  const int lda = g.lda;
  const long long a_bytes = g.a_bytes;
  const float *__restrict__ B = g.B;
  const int ldb = g.ldb;
  const long long b_bytes = g.b_bytes;
  const float *__restrict__ bias = g.bias;
  const int bias_rows = g.bias_rows;
  const float *__restrict__ Cadd = g.Cadd;
  const int ldadd = g.ldadd;
  float *__restrict__ C = g.C;
  const long long c_bytes = g.c_bytes;
  const int ldc = g.ldc;
  const GemmCols cols = g.cols;
  const int M = g.M, N = g.N, K = g.K, kper = g.kper, relu = g.relu;
  float *__restrict__ rs = g.rs;
  float *__restrict__ part = g.part;
  unsigned int *__restrict__ cnt = g.cnt;
  // rs != null (only !AK, !BKC, unbatched): B gets a logical column N of ones, so column N of
  // the product is the row sum of A over k — rs[m] = sum_k A(m, k), the bias gradient of a
  // linear layer taken by its weight-gradient GEMM (no separate column-sum launches)
  constexpr int BM = CFG::BM, BN = CFG::BN;
  constexpr int GA = BM / 32, GB = BN / 32;       // 32-row load groups per operand tile
  float(*As)[BM][G_LDW] = reinterpret_cast<float(*)[BM][G_LDW]>(lds);
  float(*Bs)[BN][G_LDW] = reinterpret_cast<float(*)[BN][G_LDW]>(lds + 2 * BM * G_LDW);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int m0 = by * BM, n0 = bx * BN;
  const int split = bz;
  const int ksteps = (K + G_BK - 1) / G_BK;
  const int kbeg = split * kper;
  const int kend = min(ksteps, kbeg + kper);
  const int nk = max(0, kend - kbeg);
  const __amdgpu_buffer_rsrc_t ra_ = rsrc(A, a_bytes), rb_ = rsrc(B, b_bytes);

  // An operand tile is groups of 32 rows x 32 k; per group a thread loads 4 values:
  // k-contiguous -> (row tid/8, k quad tid%8), one float4 / two float2 when aligned;
  // row-contiguous -> (row tid%32, k quad tid/32), lanes coalesced along the row.
  const int ar = AK ? tid >> 3 : tid & 31, aq = AK ? tid & 7 : tid >> 5;
  const int br = BKC ? tid >> 3 : tid & 31, bq = BKC ? tid & 7 : tid >> 5;

  // column-batched B: this thread's load column is fixed, so its image offset is too
  long long bcol_off[GB];
  bool bone[GB];
#pragma unroll
  for (int i = 0; i < GB; ++i) {
    const int n = min(n0 + 32 * i + br, N - 1);
    bcol_off[i] = cols.hw ? (long long)(n / cols.hw) * cols.b_img + n % cols.hw : n;
    bone[i] = !BKC && rs && n0 + 32 * i + br == N;
  }

  // One step of register lookahead: the next K-step's loads are issued before this step's
  // MFMAs and written to the other LDS buffer after them.  (Deeper register pipelines, 2 and
  // 3 steps, measured 4-5 % slower: the extra registers cost a wave per SIMD.)
  float ra[GA][4], rb[GB][4];
  // Loads are unconditional and branch-free: the row index is clamped into the matrix (rows
  // past M / N only feed outputs that are never stored) and k into the buffer; values at
  // k >= K are zeroed with an integer mask when the registers are written to LDS (after the
  // step's MFMAs, so the loads stay in flight).  The vector width is a template parameter: a
  // run-time width / K-tail switch made hipcc branch around every load group and wait
  // vmcnt(0) before the next one, serialising each K-step's loads (round 3, from the ISA).
  // A vector load at the K tail may read past the row (masked) or the buffer (reads 0).
  auto load_k = [&](float *regs, const __amdgpu_buffer_rsrc_t &rs, auto vec_c, long long base,
                    int k) {  // 4 k-contiguous values at base + k
    constexpr int vec = decltype(vec_c)::value;
    if constexpr (vec == 2) {
      const float4 v = bload4(rs, (int)((base + k) * 4));
      regs[0] = v.x; regs[1] = v.y; regs[2] = v.z; regs[3] = v.w;
    } else if constexpr (vec == 1) {
      const float2 v0 = bload2(rs, (int)((base + k) * 4)), v1 = bload2(rs, (int)((base + k + 2) * 4));
      regs[0] = v0.x; regs[1] = v0.y; regs[2] = v1.x; regs[3] = v1.y;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) regs[j] = bload(rs, (int)((base + min(k + j, K - 1)) * 4));
    }
  };
  auto load_tiles = [&](float (&xa)[GA][4], float (&xb)[GB][4], int ks_in) {
    const int k0 = min(ks_in, kend - 1) * G_BK;  // past the range: re-read, never stored
#pragma unroll
    for (int i = 0; i < GA; ++i) {
      const int row = min(m0 + 32 * i + ar, M - 1);
      const int k = k0 + 4 * aq;
      if (AK) {
        load_k(xa[i], ra_, std::integral_constant<int, AVEC>{}, (long long)row * lda, k);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          xa[i][j] = bload(ra_, (int)(((long long)min(k + j, K - 1) * lda + row) * 4));
      }
    }
#pragma unroll
    for (int i = 0; i < GB; ++i) {
      const int k = k0 + 4 * bq;
      if (BKC) {
        const int row = min(n0 + 32 * i + br, N - 1);
        load_k(xb[i], rb_, std::integral_constant<int, BVEC>{}, (long long)row * ldb, k);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = bload(rb_, (int)(((long long)min(k + j, K - 1) * ldb + bcol_off[i]) * 4));
          xb[i][j] = bone[i] ? 1.f : v;
        }
      }
    }
  };
  // LDS writes: regs -> k-contiguous rows; the zero mask for k >= K applied here
  auto store_tiles = [&](float (&xa)[GA][4], float (&xb)[GB][4], int buf, int ks) {
    const int k0 = ks * G_BK;
    const bool full = k0 + G_BK <= K;  // uniform
#pragma unroll
    for (int i = 0; i < GA; ++i) {
      if (!full)
#pragma unroll
        for (int j = 0; j < 4; ++j) xa[i][j] = kmask(xa[i][j], k0 + 4 * aq + j < K);
      *reinterpret_cast<float4 *>(&As[buf][32 * i + ar][4 * aq]) =
          make_float4(xa[i][0], xa[i][1], xa[i][2], xa[i][3]);
    }
#pragma unroll
    for (int i = 0; i < GB; ++i) {
      if (!full)
#pragma unroll
        for (int j = 0; j < 4; ++j) xb[i][j] = kmask(xb[i][j], k0 + 4 * bq + j < K);
      *reinterpret_cast<float4 *>(&Bs[buf][32 * i + br][4 * bq]) =
          make_float4(xb[i][0], xb[i][1], xb[i][2], xb[i][3]);
    }
  };

  // wave (wm, wn) owns rows 32 TM wm + 32 u and columns 32 TN wn + 32 t
  g_f32x16 acc[TM][TN];
#pragma unroll
  for (int u = 0; u < TM; ++u)
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[u][t] = g_f32x16{0};
  const int li = lane & 31, lh = lane >> 5;
  // lane half h supplies k = 16h .. 16h+15 to the 16 MFMAs of a step
  auto compute = [&](int buf) {
    float a[TM][16], b[TN][16];
#pragma unroll
    for (int u = 0; u < TM; ++u) {
      const float *p = &As[buf][32 * TM * wm + 32 * u + li][16 * lh];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 x = *reinterpret_cast<const float4 *>(p + 4 * q);
        a[u][4 * q] = x.x; a[u][4 * q + 1] = x.y; a[u][4 * q + 2] = x.z; a[u][4 * q + 3] = x.w;
      }
    }
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const float *p = &Bs[buf][32 * TN * wn + 32 * t + li][16 * lh];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 x = *reinterpret_cast<const float4 *>(p + 4 * q);
        b[t][4 * q] = x.x; b[t][4 * q + 1] = x.y; b[t][4 * q + 2] = x.z; b[t][4 * q + 3] = x.w;
      }
    }
    if (OP == 0) {
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
#pragma unroll
        for (int u = 0; u < TM; ++u)
#pragma unroll
          for (int t = 0; t < TN; ++t)
            acc[u][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][kk], b[t][kk], acc[u][t], 0, 0, 0);
    } else {
      // lane half h supplies k = 16h + 8 blk + j to MFMA blk (element j): one consistent
      // permutation of the step's 32 k for both operands
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        g_bf16x8 ab[TM], bb[TN];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
          for (int u = 0; u < TM; ++u) ab[u][j] = (__bf16)a[u][8 * blk + j];
#pragma unroll
          for (int t = 0; t < TN; ++t) bb[t][j] = (__bf16)b[t][8 * blk + j];
        }
#pragma unroll
        for (int u = 0; u < TM; ++u)
#pragma unroll
          for (int t = 0; t < TN; ++t)
            acc[u][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab[u], bb[t], acc[u][t], 0, 0, 0);
      }
    }
  };
  if (nk > 0) {
    load_tiles(ra, rb, kbeg);
    store_tiles(ra, rb, 0, kbeg);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      load_tiles(ra, rb, kbeg + kt + 1);  // past the range: re-read, never stored
      // keep the loads at the top of the step: hipcc otherwise sinks them behind half the
      // MFMAs, leaving half a step to cover their latency before the LDS write waits on them
      __builtin_amdgcn_sched_barrier(0);
      compute(kt & 1);
      // all of the step's MFMAs before the LDS write (hipcc otherwise hoists the write, and its
      // wait on the loads, into the middle of them); unconditional: the last step's copy lands
      // in the idle buffer and is never read (a conditional store lets hipcc sink loads into
      // its branch, behind the MFMAs)
      __builtin_amdgcn_sched_barrier(0);
      store_tiles(ra, rb, (kt + 1) & 1, min(kbeg + kt + 1, kend - 1));
      __syncthreads();
    }
  }

  // epilogue: C/D layout col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
  // gridDim.z > 1: raw partial sums into part[split][M][Nw] (dense, unbatched); with `cnt`
  // (the in-launch fold) they are stored write-through, the tile's last-arriving split sums
  // every slab in split order (k_gemm_reduce's order) and runs the final epilogue below; with
  // no `cnt` k_gemm_reduce does that in a launch of its own.
  const int Nw = rs ? N + 1 : N;  // split-K partials carry the row-sum column
  if (g.gz > 1) {
    const long long MNw = (long long)M * Nw;
    const __amdgpu_buffer_rsrc_t rp = rsrc(part + split * MNw, 4LL * MNw);
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const int n = n0 + 32 * TN * wn + 32 * t + li;
      const bool nok = n < N || (rs && n == N);
#pragma unroll
      for (int u = 0; u < TM; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + 32 * TM * wm + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const int off = (nok && m < M) ? (m * Nw + n) * 4 : OOR;
          if (cnt) bstore_sc1(rp, off, acc[u][t][r]);
          else bstore(rp, off, acc[u][t][r]);
        }
    }
    if (!cnt) return;
    handoff_drain();
    if (!handoff_arrive(cnt + bx + g.gx * by, g.gz, s_last)) return;
    const __amdgpu_buffer_rsrc_t rall = rsrc(part, 4LL * g.gz * MNw);
    for (int k = 0; k < g.gz; ++k) {
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const int n = n0 + 32 * TN * wn + 32 * t + li;
        const bool nok = n < N || (rs && n == N);
#pragma unroll
        for (int u = 0; u < TM; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = m0 + 32 * TM * wm + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const float v = bload_sc1(rall, (nok && m < M) ? (int)((k * MNw + m * Nw + n) * 4) : OOR);
            acc[u][t][r] = k == 0 ? v : acc[u][t][r] + v;
          }
      }
    }
  }
  const bool final_ = true;
  float *dst = C;
  const int ldd = ldc;
  const bool batched = cols.hw > 0;
  // edges: buffer stores with out-of-range offsets are dropped; the epilogue's optional
  // inputs are behind uniform branches, and the 16 Cadd values of a tile are loaded together
  const __amdgpu_buffer_rsrc_t rd = rsrc(dst, c_bytes);
  const __amdgpu_buffer_rsrc_t rrs = rsrc(rs, rs ? 4LL * M : 0);
  const __amdgpu_buffer_rsrc_t rc =
      rsrc(Cadd, Cadd ? (batched ? c_bytes : 4LL * ((long long)(M - 1) * ldadd + N)) : 0);
  const bool add_c = final_ && Cadd != nullptr, add_b = final_ && bias != nullptr;
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int n = n0 + 32 * TN * wn + 32 * t + li;
    const bool nok = n < N;
    const bool rsc = rs && n == N;
    const long long cbase = batched ? (long long)(n / cols.hw) * cols.c_img + n % cols.hw : n;
    const float bn_ = (add_b && !bias_rows) ? bias[min(n, N - 1)] : 0.f;
#pragma unroll
    for (int u = 0; u < TM; ++u) {
      float cv[16];
      if (add_c) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + 32 * TM * wm + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const long long off = batched ? cbase + (long long)m * ldd : (long long)m * ldadd + n;
          cv[r] = bload(rc, (nok && m < M) ? (int)(off * 4) : OOR);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + 32 * TM * wm + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float v = acc[u][t][r];
        if (add_b) v += bias_rows ? bias[min(m, M - 1)] : bn_;
        if (add_c) v += cv[r];
        if (final_ && relu) v = fmaxf(v, 0.f);
        bstore(rd, (nok && m < M) ? (int)((cbase + (long long)m * ldd) * 4) : OOR, v);
        if (rs) bstore(rrs, (rsc && m < M) ? m * 4 : OOR, v);
      }
    }
  }
}

template <bool AK, bool BKC, int WM, int TM, int TN, int AVEC, int BVEC, int OP = 0>
__global__ void __launch_bounds__(256) k_gemm(GemmArgs g) {
  typedef GemmCfg<AK, BKC, WM, TM, TN, AVEC, BVEC, OP> CFG;
  __shared__ __attribute__((aligned(16))) float lds[CFG::LDS_FLOATS];
  __shared__ int s_last;
  gemm_block<CFG>(g, blockIdx.x, blockIdx.y, blockIdx.z, lds, &s_last);
}

// Two independent GEMM problems in one launch (a linear layer's input gradient and its
// weight + bias gradient, e2ep_linear_bwd): blocks [0, n1) run problem 1, the rest problem 2,
// each with its own tile grid, splits and fold counters.  One launch instead of two on forked
// streams: in a replayed graph a fork / join costs ~5 + ~10 us of idle GPU (scripts/
// step_sequence.py), more than either product of the control decoder takes.
template <class C1, class C2>
__global__ void __launch_bounds__(256) k_gemm_pair(GemmArgs g1, GemmArgs g2) {
  constexpr int L = C1::LDS_FLOATS > C2::LDS_FLOATS ? C1::LDS_FLOATS : C2::LDS_FLOATS;
  __shared__ __attribute__((aligned(16))) float lds[L];
  __shared__ int s_last;
  // the first problem's blocks first (the reverse order was within noise,
  // profiles/r04/linear_pair_order_ab.txt; the switch is retired)
  const int n1 = g1.gx * g1.gy * g1.gz;
  int id = (int)blockIdx.x;
  if (id < n1) {
    gemm_block<C1>(g1, id % g1.gx, (id / g1.gx) % g1.gy, id / (g1.gx * g1.gy), lds, &s_last);
  } else {
    id -= n1;
    gemm_block<C2>(g2, id % g2.gx, (id / g2.gx) % g2.gy, id / (g2.gx * g2.gy), lds, &s_last);
  }
}

// C[m][n] = sum over splits in order (+ bias) (+ Cadd) (ReLU).  V = 4: four consecutive
// elements per thread with 16-byte loads / stores (plain dense C, column bias, M*N % 4 == 0);
// V = 1 handles column-batched C (Cadd in C's layout) and row bias.
template <int V>
__global__ void __launch_bounds__(256)
    k_gemm_reduce(const float *__restrict__ part, int splits, int M, int N,
                  const float *__restrict__ bias, int bias_rows, const float *__restrict__ Cadd,
                  int ldadd, float *__restrict__ C, int ldc, GemmCols cols, int relu,
                  float *__restrict__ rs) {
  // rs: the partials are M x (N + 1), column N = row sums of A (V = 1 only)
  const int Nw = rs ? N + 1 : N;
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  const long long MN = (long long)M * Nw;
  if (i >= MN) return;
  float s[V];
  if (V == 4) {
    float4 a = *reinterpret_cast<const float4 *>(part + i);
    s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
    for (int k = 1; k < splits; ++k) {
      a = *reinterpret_cast<const float4 *>(part + k * MN + i);
      s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w;
    }
  } else {
    s[0] = part[i];
    for (int k = 1; k < splits; ++k) s[0] += part[k * MN + i];
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const long long e = i + v;
    const int m = (int)(e / Nw), n = (int)(e - (long long)m * Nw);
    if (V == 1 && rs && n == N) {
      rs[m] = s[v];
      return;
    }
    const long long off = cols.hw ? (long long)(n / cols.hw) * cols.c_img + n % cols.hw +
                                        (long long)m * ldc
                                  : (long long)m * ldc + n;
    if (bias) s[v] += bias[bias_rows ? m : n];
    if (Cadd) s[v] += Cadd[cols.hw ? off : (long long)m * ldadd + n];
    if (relu) s[v] = fmaxf(s[v], 0.f);
    if (V == 1) C[off] = s[v];
  }
  if (V == 4) *reinterpret_cast<float4 *>(C + i) = make_float4(s[0], s[1], s[2], s[3]);
}

// Skinny GEMM for the forward layout with few rows (M <= g_skinny_rows, at most SK_ROWS: the
// control decoder's 14 token rows in C5 predict): C[m][n] = sum_k A[m*lda + k]
// B[n*ldb + k] (+ bias[n]) (+ Cadd) (ReLU).  One block per (output column n, chunk of
// SK_MAXM rows); lanes stride k (float2 when lda, ldb are even and the bases 8-byte aligned),
// each lane keeps SK_MAXM partial dot products; fixed-order wave, then block, reductions.  The
// MFMA tiles (32 x 128 at the least) left those launches a chain of K-steps on a dozen blocks
// (15 us for a 14 x 2048 x 258 product).
constexpr int SK_MAXM = 16, SK_ROWS = 128;
template <int V>
__global__ void __launch_bounds__(256) k_gemm_skinny(
    const float *__restrict__ A, int lda, const float *__restrict__ B, int ldb,
    const float *__restrict__ bias, const float *__restrict__ Cadd, int ldadd,
    float *__restrict__ C, int ldc, int M, int N, int K, int relu) {
  __shared__ float red[4][SK_MAXM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x;
  const int m0 = blockIdx.y * SK_MAXM;
  A += (size_t)m0 * lda;
  C += (size_t)m0 * ldc;
  if (Cadd) Cadd += (size_t)m0 * ldadd;
  M = min(M - m0, SK_MAXM);
  float acc[SK_MAXM];
#pragma unroll
  for (int m = 0; m < SK_MAXM; ++m) acc[m] = 0.f;
  const float *brow = B + (size_t)n * ldb;
  for (int k = (wave * 64 + lane) * V; k < K; k += 256 * V) {
    if (V == 2 && k + 1 < K) {
      const float2 b = *reinterpret_cast<const float2 *>(brow + k);
      float2 a[SK_MAXM];
#pragma unroll
      for (int m = 0; m < SK_MAXM; ++m)
        a[m] = *reinterpret_cast<const float2 *>(A + (size_t)min(m, M - 1) * lda + k);
#pragma unroll
      for (int m = 0; m < SK_MAXM; ++m) {
        acc[m] = fmaf(a[m].x, b.x, acc[m]);
        acc[m] = fmaf(a[m].y, b.y, acc[m]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (k + j >= K) break;
        const float b = brow[k + j];
#pragma unroll
        for (int m = 0; m < SK_MAXM; ++m)
          acc[m] = fmaf(A[(size_t)min(m, M - 1) * lda + k + j], b, acc[m]);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < SK_MAXM; ++m) {
    const float v = wave_sum(acc[m]);
    if (lane == 0) red[wave][m] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < M) {
    const int m = threadIdx.x;
    float v = (red[0][m] + red[1][m]) + (red[2][m] + red[3][m]);
    if (bias) v += bias[n];
    if (Cadd) v += Cadd[(size_t)m * ldadd + n];
    if (relu) v = fmaxf(v, 0.f);
    C[(size_t)m * ldc + n] = v;
  }
}

// ---- host: one plan per product (gemm_plan), one dispatcher family, one entry check ----------
namespace {  // (conv.hip has a GemmPlan of its own for its implicit GEMMs)

// Block tiles (wm waves along M, wave tile 32 tm x 32 tn):
//   1: 64 x 64 (2 x 2 waves, 32 x 32)     2: 32 x 128 (1 x 4, 32 x 32)
//   3: 128 x 128 (2 x 2, 64 x 64)         4: 64 x 128 (2 x 2, 32 x 64)
//   5: 128 x 64 (2 x 2, 64 x 32)          6: 64 x 256 (1 x 4, 64 x 64)
// (the larger tiles measured no faster on the C2 shapes, scripts/bench_gemm.py --sweep:
// profiles/r02/gemm_sweep_tiles.json; they stay selectable for other shapes)
struct GemmTile {
  int bm, bn;
};
GemmTile tile_dims(int tile) {
  const GemmTile dims[7] = {{64, 64}, {64, 64}, {32, 128}, {128, 128}, {64, 128}, {128, 64}, {64, 256}};
  return dims[tile >= 1 && tile <= 6 ? tile : 1];
}

// The process-wide settings below and e2ep_tune keys 4 and 28 are read by gemm_plan alone.
int g_force_tile = 0, g_force_splits = 0;  // e2ep_gemm_force; 0: automatic
// K-steps per split for grids under 64 blocks (e2ep_gemm_split_min).  8, 4 and 2 measured
// the same C2 step within noise (25.52 / 25.49 / 25.44 ms, profiles/r02/session6/
// gemm_split_min_ab.txt): the default stays 8.
int g_split_min_small = 8;
// e2ep_gemm_skinny: few-row forward products up to this M.  16 (the decoder at B = 1): C5
// predict fp16 4.84 -> 4.28 ms p50; the C2 step's 112-row decoder measured slower on it (25.66
// vs 25.39 ms/step, profiles/r02/session6/skinny_ab.txt), so it stays on the MFMA tiles.
int g_skinny_rows = 16;
// operand precision of k_gemm (e2ep_gemm_precision): 0 fp32, 1 bf16 (C3)
int g_gemm_precision = 0;

// vector loads along k for k-contiguous operands: 2 = float4 (rows 16-byte aligned), 1 =
// float2 (8-byte aligned: the d = 258 rows).  Row-contiguous operands stay on dword loads
// (lanes consecutive along the row): a float2 row-pair variant measured 1.2 - 1.5x slower on
// the weight-gradient shapes.
int vec_of(bool kc, int ld, const void *ptr) {
  if (!kc) return 0;
  if (ld % 4 == 0 && ((uintptr_t)ptr & 15) == 0) return 2;
  return ld % 2 == 0 && ((uintptr_t)ptr & 7) == 0 ? 1 : 0;
}

enum GemmRoute {
  GEMM_SKINNY,  // k_gemm_skinny<skinny_v>; the tile fields below are still filled (ws_bytes)
  GEMM_TILES,   // k_gemm, one split, epilogue in the launch
  GEMM_FOLD,    // k_gemm, K split, the last-arriving split of a tile folds (e2ep_tune key 28 = 2)
  GEMM_REDUCE,  // k_gemm, K split, then k_gemm_reduce<reduce_v>
};

struct GemmPlan {  // everything the host decides about one product, decided once by gemm_plan()
  GemmRoute route;
  int op;    // operand precision of k_gemm (the skinny kernel stays fp32)
  int tile;  // 1..6; bf16 operands: a forced 3..6 runs as 1 (clamped after the splits are set)
  int nx;    // logical columns planned for: N + 1 with a row sum (the ones column)
  // Automatic: toward e2ep_tune key 4 workgroups, at most 8 ways and >= 8 K-steps each; grids
  // under 64 blocks (the decoder's 112-row products: a chain of K-steps on a dozen blocks) at
  // most 16 ways and >= e2ep_gemm_split_min K-steps.  Forced splits are clamped to the K-step
  // count.  Then rebalanced, kper = ceil(ksteps / splits), splits = ceil(ksteps / kper): no
  // split is empty (a forced 3 over 4 K-steps runs as 2).
  int splits, kper;
  int gx, gy;  // column tiles x row tiles (x splits = the k_gemm grid)
  // Split-K partials, splits * M * nx floats (0 unsplit): a function of the splits alone, so
  // neither precision nor fold mode changes it.  Filled on the skinny route too, which never
  // touches a workspace: e2ep_gemm_workspace knows no layout, and e2ep_gemm demands what it says.
  size_t ws_bytes;
  int avec, bvec;  // vec_of each operand (0 for a row-contiguous one)
  int skinny_v;    // 2: float2 along k (lda, ldb even, A and B 8-byte aligned), else 1
  int reduce_v;    // 4: float4 reduce (dense C and Cadd, column bias, no row sum, 16-byte C), else 1
  // Can be half of a k_gemm_pair launch: an automatic plan (tile 1 or 2) that is unsplit or
  // folds in the launch.  A pair needs both halves pairable and, for each split half, counters.
  bool pairable;
};

GemmPlan gemm_plan(const GemmProblem &q) {
  GemmPlan p{};
  const bool forced = g_force_tile > 0;  // benchmarking override (e2ep_gemm_force)
  const int M = q.M, ksteps = cdiv(q.K, G_BK);
  p.op = g_gemm_precision;
  p.nx = q.rs ? q.N + 1 : q.N;
  // automatic: 32 x 128 when 32-row tiles pad M less than 64-row ones (M = 32, 112, 144, 160,
  // 336 ...), else 64 x 64 (scripts/bench_gemm.py --sweep / --conv)
  p.tile = forced ? g_force_tile : cdiv(M, 32) * 32 < cdiv(M, 64) * 64 ? 2 : 1;
  if (forced) {
    p.splits = std::max(1, std::min(g_force_splits, ksteps));
  } else {
    const GemmTile t = tile_dims(p.tile);
    const long long blocks = (long long)cdiv(M, t.bm) * cdiv(p.nx, t.bn);
    const int smin = blocks < 64 ? g_split_min_small : 8;
    const int cap = std::min(blocks < 64 ? 16 : 8, std::max(1, ksteps / smin));
    p.splits = (int)std::min<long long>(
        cap, std::max(1LL, (long long)cdiv(g_tune[TUNE_GEMM_SPLIT_TARGET], blocks)));
  }
  p.kper = cdiv(ksteps, p.splits);
  p.splits = cdiv(ksteps, p.kper);
  if (p.op == 1 && p.tile != 1 && p.tile != 2) p.tile = 1;
  const GemmTile t = tile_dims(p.tile);
  p.gx = cdiv(p.nx, t.bn), p.gy = cdiv(M, t.bm);
  p.ws_bytes = p.splits > 1 ? (size_t)p.splits * M * p.nx * sizeof(float) : 0;
  const bool skinny = q.ak && q.bk && !q.bias_rows && q.cols.hw == 0 && !q.rs && M <= g_skinny_rows && !forced;
  p.route = skinny ? GEMM_SKINNY : p.splits == 1 ? GEMM_TILES
            : g_tune[TUNE_SPLITK_FOLD] == 2 ? GEMM_FOLD : GEMM_REDUCE;
  p.avec = vec_of(q.ak, q.lda, q.A), p.bvec = vec_of(q.bk, q.ldb, q.B);
  p.skinny_v = q.lda % 2 == 0 && q.ldb % 2 == 0 && (((uintptr_t)q.A | (uintptr_t)q.B) & 7) == 0 ? 2 : 1;
  p.reduce_v = !q.rs && (long long)M * q.N % 4 == 0 && q.ldc == q.N && q.cols.hw == 0 &&
                       !q.bias_rows && (!q.Cadd || q.ldadd == q.N) && ((uintptr_t)q.C & 15) == 0
                   ? 4 : 1;
  p.pairable = !forced && (p.tile == 1 || p.tile == 2) && p.route != GEMM_SKINNY && p.route != GEMM_REDUCE;
  return p;
}

GemmArgs gemm_args(const GemmProblem &q, const GemmPlan &p, void *workspace, unsigned int *cnt) {
  return GemmArgs{q.A, q.lda, q.a_bytes, q.B, q.ldb, q.b_bytes, q.bias, q.bias_rows ? 1 : 0,
                  q.Cadd, q.ldadd, q.C, q.c_bytes, q.ldc, q.cols, q.M, q.N, q.K, p.kper, q.relu,
                  q.rs, p.splits > 1 ? static_cast<float *>(workspace) : nullptr, cnt, p.gx, p.gy,
                  p.splits};
}

// ---- template dispatch: f is a generic lambda (integral constants: common.h IntC) -----------
template <class F> void with_bool(bool b, F f) {
  if (b) f(std::true_type());
  else f(std::false_type());
}
// f(VEC): 2, 1 or 0 for a k-contiguous operand (KC), 0 alone for a row-contiguous one
template <bool KC, class F> void with_vec(int vec, F f) {
  if constexpr (KC) {
    if (vec == 2) return f(IntC<2>());
    if (vec == 1) return f(IntC<1>());
  }
  f(IntC<0>());
}
// f(WM): waves along M of the two 32 x 32-wave-tile blocks, tile 2 (32 x 128) or tile 1 (64 x 64)
template <class F> void with_wm(int tile, F f) {
  if (tile == 2) f(IntC<1>());
  else f(IntC<2>());
}
// f(WM, TM, TN, OP): the six fp32 tiles, the two bf16 ones
template <class F> void with_tile_op(int tile, int op, F f) {
  IntC<0> o;
  IntC<1> i1;
  IntC<2> i2;
  if (op == 1) with_wm(tile, [&](auto wm) { f(wm, i1, i1, i1); });
  else if (tile == 2) f(i1, i1, i1, o);
  else if (tile == 3) f(i2, i2, i2, o);
  else if (tile == 4) f(i2, i1, i2, o);
  else if (tile == 5) f(i2, i2, i1, o);
  else if (tile == 6) f(i1, i2, i2, o);
  else f(i2, i1, i1, o);
}

void launch_tiles(const GemmProblem &q, const GemmPlan &p, const GemmArgs &ga, hipStream_t s) {
  const dim3 grid(p.gx, p.gy, p.splits);
  with_bool(q.ak, [&](auto ak) {
    with_bool(q.bk, [&](auto bk) {
      constexpr bool AK = decltype(ak)::value, BK = decltype(bk)::value;
      with_vec<AK>(p.avec, [&](auto av) {
        with_vec<BK>(p.bvec, [&](auto bv) {
          with_tile_op(p.tile, p.op, [&](auto wm, auto tm, auto tn, auto op) {
            hipLaunchKernelGGL((k_gemm<AK, BK, decltype(wm)::value, decltype(tm)::value,
                                       decltype(tn)::value, decltype(av)::value,
                                       decltype(bv)::value, decltype(op)::value>),
                               grid, dim3(256), 0, s, ga);
          });
        });
      });
    });
  });
}

// k_gemm_pair for (input gradient: A k-contiguous, B row-contiguous) + (weight gradient with
// the row-sum column: both row-contiguous), over the tiles / vector width / precision
void launch_pair(const GemmPlan &p1, const GemmArgs &g1, const GemmPlan &p2, const GemmArgs &g2,
                 hipStream_t s) {
  const dim3 grid(g1.gx * g1.gy * g1.gz + g2.gx * g2.gy * g2.gz);
  with_bool(p1.op == 1, [&](auto op) {
    with_wm(p1.tile, [&](auto wm1) {
      with_vec<true>(p1.avec, [&](auto av1) {
        with_wm(p2.tile, [&](auto wm2) {
          constexpr int OP = decltype(op)::value ? 1 : 0;
          hipLaunchKernelGGL(
              (k_gemm_pair<GemmCfg<true, false, decltype(wm1)::value, 1, 1, decltype(av1)::value, 0, OP>,
                           GemmCfg<false, false, decltype(wm2)::value, 1, 1, 0, 0, OP>>),
              grid, dim3(256), 0, s, g1, g2);
        });
      });
    });
  });
}

int gemm_launch(const GemmProblem &q, const GemmPlan &p, void *workspace, hipStream_t s) {
  if (p.route == GEMM_SKINNY) {
    const dim3 grid(q.N, cdiv(q.M, SK_MAXM));
    with_bool(p.skinny_v == 2, [&](auto v2) {
      hipLaunchKernelGGL(k_gemm_skinny<(decltype(v2)::value ? 2 : 1)>, grid, dim3(256), 0, s, q.A,
                         q.lda, q.B, q.ldb, q.bias, q.Cadd, q.ldadd, q.C, q.ldc, q.M, q.N, q.K, q.relu);
    });
    return 0;
  }
  if (p.splits > 1 && !workspace) {
    set_error("gemm: workspace of e2ep_gemm_workspace() bytes required");
    return E2EP_EINVAL;
  }
  // a launch that wants the fold but gets no counters reduces in a second launch instead
  unsigned int *cnt = p.route == GEMM_FOLD ? handoff_slots(p.gx * p.gy, s) : nullptr;
  launch_tiles(q, p, gemm_args(q, p, workspace, cnt), s);
  if (p.splits > 1 && !cnt) {
    const long long MN = (long long)q.M * p.nx;
    with_bool(p.reduce_v == 4, [&](auto v4) {
      constexpr int V = decltype(v4)::value ? 4 : 1;
      hipLaunchKernelGGL(k_gemm_reduce<V>, dim3(cdiv(MN / V, 256)), dim3(256), 0, s,
                         static_cast<const float *>(workspace), p.splits, q.M, q.N, q.bias,
                         q.bias_rows ? 1 : 0, q.Cadd, q.ldadd, q.C, q.ldc, q.cols, q.relu, q.rs);
    });
  }
  return 0;
}

// bytes from an operand's base to the end of its last row: `rows` rows of `cols` floats, ld apart
long long extent_bytes(int rows, int ld, int cols) { return 4LL * ((long long)(rows - 1) * ld + cols); }

// a plain-matrix problem's operand extents from its dimensions and leading dimensions
void set_extents(GemmProblem &q) {
  q.a_bytes = q.ak ? extent_bytes(q.M, q.lda, q.K) : extent_bytes(q.K, q.lda, q.M);
  q.b_bytes = q.bk ? extent_bytes(q.N, q.ldb, q.K) : extent_bytes(q.K, q.ldb, q.N);
  q.c_bytes = extent_bytes(q.M, q.ldc, q.N);
}

// An entry point's check of one (plain-matrix) problem: leading dimensions, the workspace its
// plan needs, 32-bit byte offsets.
int gemm_check(const char *who, const GemmProblem &q, const GemmPlan &p, const void *ws, size_t ws_bytes) {
  E2EP_REQUIRE(q.lda >= (q.ak ? q.K : q.M) && q.ldb >= (q.bk ? q.K : q.N) && q.ldc >= q.N &&
                   (!q.Cadd || q.ldadd >= q.N),
               E2EP_EINVAL, "%s: leading dimension too small", who);
  E2EP_REQUIRE(!p.ws_bytes || (ws && ws_bytes >= p.ws_bytes), E2EP_EINVAL,
               "%s: workspace %zu bytes < %zu the launch plan of the %d x %d x %d product needs (query "
               "e2ep_gemm_workspace / e2ep_gemm_rowsum_workspace after setting precision / tunables)",
               who, ws_bytes, p.ws_bytes, q.M, q.N, q.K);
  const long long lim = 0x7fffffffLL;
  E2EP_REQUIRE(q.a_bytes < lim && q.b_bytes < lim && q.c_bytes < lim &&
                   (!q.Cadd || extent_bytes(q.M, q.ldadd, q.N) < lim) &&
                   (!q.rs || 4LL * q.M * (q.N + 1) * 8 < lim),
               E2EP_ERANGE, "%s: operand larger than 2 GB", who);
  return 0;
}

}  // namespace

int gemm_run(const GemmProblem &q, void *workspace, hipStream_t s) {
  if (q.rs && (q.ak || q.bk || q.cols.hw)) {
    set_error("gemm: the row sum of A needs a k-major A, a row-contiguous B, unbatched C");
    return E2EP_EINVAL;
  }
  return gemm_launch(q, gemm_plan(q), workspace, s);
}

size_t gemm_ws(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  GemmProblem q{};
  q.M = M, q.N = N, q.K = K;
  return gemm_plan(q).ws_bytes;
}

}  // namespace e2ep

using namespace e2ep;

extern "C" {

int e2ep_linear_bwd(const float *dy, int ldy, const float *x, int ldx, const float *w, int ldw,
                    const float *gskip, int ldskip, float *dx, int lddx, float *dw, int lddw,
                    float *db, int M, int N, int K, void *ws_dx, size_t ws_dx_bytes, void *ws_dw,
                    size_t ws_dw_bytes, void *stream) {
  E2EP_REQUIRE(dy && x && w && dx && dw && db && M > 0 && N > 0 && K > 0, E2EP_EINVAL,
               "e2ep_linear_bwd: bad arguments M=%d N=%d K=%d", M, N, K);
  // dX[M][K] = dY[M][N] W[N][K] (+ gskip);  dW[N][K] = dY^T X with db[N] = row sums of dY^T
  GemmProblem qx{}, qw{};
  qx.A = dy, qx.lda = ldy, qx.ak = true, qx.B = w, qx.ldb = ldw, qx.C = dx, qx.ldc = lddx;
  qx.Cadd = gskip, qx.ldadd = ldskip;
  qx.M = M, qx.N = K, qx.K = N;
  qw.A = dy, qw.lda = ldy, qw.B = x, qw.ldb = ldx, qw.C = dw, qw.ldc = lddw, qw.rs = db;
  qw.M = N, qw.N = K, qw.K = M;
  set_extents(qx), set_extents(qw);
  const GemmPlan px = gemm_plan(qx), pw = gemm_plan(qw);
  if (int rc = gemm_check("e2ep_linear_bwd", qx, px, ws_dx, ws_dx_bytes)) return rc;
  if (int rc = gemm_check("e2ep_linear_bwd", qw, pw, ws_dw, ws_dw_bytes)) return rc;
  hipStream_t s = as_stream(stream);
  if (px.pairable && pw.pairable) {
    // counters only now that both halves pair; a split half that gets none: two launches below
    unsigned int *cx = nullptr, *cw = nullptr;
    if ((px.splits == 1 || (cx = handoff_slots(px.gx * px.gy, s))) &&
        (pw.splits == 1 || (cw = handoff_slots(pw.gx * pw.gy, s)))) {
      launch_pair(px, gemm_args(qx, px, ws_dx, cx), pw, gemm_args(qw, pw, ws_dw, cw), s);
      return launch_status("e2ep_linear_bwd");
    }
  }
  // fallback (benchmark-forced tiles, folds off): the two launches in order on one stream
  if (int rc = gemm_launch(qx, px, ws_dx, s)) return rc;
  if (int rc = gemm_launch(qw, pw, ws_dw, s)) return rc;
  return launch_status("e2ep_linear_bwd");
}

int e2ep_gemm_force(int tile, int splits, int unused) {
  (void)unused;
  E2EP_REQUIRE(tile >= 0 && tile <= 6 && splits >= 0, E2EP_EINVAL,
               "e2ep_gemm_force: tile in 1..6 (0 = automatic), splits >= 0");
  g_force_tile = tile;
  g_force_splits = splits;
  return 0;
}

int e2ep_gemm_split_min(int ksteps) {
  const int prev = g_split_min_small;
  if (ksteps > 0) g_split_min_small = ksteps;
  return prev;
}

int e2ep_gemm_precision(int precision) {
  const int prev = g_gemm_precision;
  if (precision == 0 || precision == 1) g_gemm_precision = precision;
  return prev;
}

int e2ep_gemm_skinny(int max_rows) {
  const int prev = g_skinny_rows;
  if (max_rows >= 0) g_skinny_rows = std::min(max_rows, SK_ROWS);
  return prev;
}

size_t e2ep_gemm_workspace(int M, int N, int K) { return gemm_ws(M, N, K); }
size_t e2ep_gemm_rowsum_workspace(int M, int N, int K) { return gemm_ws(M, N + 1, K); }

int e2ep_gemm(const float *A, int lda, int a_kcontig, const float *B, int ldb, int b_kcontig,
              const float *bias, const float *Cadd, int ldadd, float *C, int ldc, int M, int N,
              int K, int relu, void *workspace, size_t workspace_bytes, void *stream) {
  E2EP_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0, E2EP_EINVAL,
               "e2ep_gemm: bad arguments M=%d N=%d K=%d", M, N, K);
  GemmProblem q{};
  q.A = A, q.lda = lda, q.ak = a_kcontig, q.B = B, q.ldb = ldb, q.bk = b_kcontig, q.C = C, q.ldc = ldc;
  q.bias = bias, q.Cadd = Cadd, q.ldadd = ldadd, q.relu = relu;
  q.M = M, q.N = N, q.K = K;
  set_extents(q);
  const GemmPlan p = gemm_plan(q);
  if (int rc = gemm_check("e2ep_gemm", q, p, workspace, workspace_bytes)) return rc;
  if (int rc = gemm_launch(q, p, workspace, as_stream(stream))) return rc;
  return launch_status("e2ep_gemm");
}

int e2ep_gemm_rowsum(const float *A, int lda, const float *B, int ldb, float *C, int ldc,
                     float *rowsum, int M, int N, int K, void *workspace,
                     size_t workspace_bytes, void *stream) {
  E2EP_REQUIRE(A && B && C && rowsum && M > 0 && N > 0 && K > 0, E2EP_EINVAL,
               "e2ep_gemm_rowsum: bad arguments M=%d N=%d K=%d", M, N, K);
  GemmProblem q{};
  q.A = A, q.lda = lda, q.B = B, q.ldb = ldb, q.C = C, q.ldc = ldc, q.rs = rowsum;
  q.M = M, q.N = N, q.K = K;
  set_extents(q);
  const GemmPlan p = gemm_plan(q);
  if (int rc = gemm_check("e2ep_gemm_rowsum", q, p, workspace, workspace_bytes)) return rc;
  if (int rc = gemm_launch(q, p, workspace, as_stream(stream))) return rc;
  return launch_status("e2ep_gemm_rowsum");
}

}  // extern "C"
