// Internal interface of the strided / column-batched MFMA GEMM (gemm.hip), shared with the
// 1x1-convolution path of conv.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace e2ep {

// Column batching (1x1 convolutions, NCHW): with hw > 0, column n = (image n / hw, pixel
// n % hw); B(k, n) = B[img * b_img + k * ldb + p] and C(m, n) = C[img * c_img + m * ldc + p]
// (Cadd in C's layout).  hw must be a multiple of 32.
struct GemmCols {
  int hw;  // 0: plain matrix
  long long b_img, c_img;
};

// One product C = A B (+ bias: per column, or per row when bias_rows) (+ Cadd) (ReLU); see
// gemm.hip.  Filled by name (GemmProblem q{}; q.A = ...): what is left out is absent.
struct GemmProblem {
  const float *A;  // A(m, k) = ak ? A[m * lda + k] : A[k * lda + m]
  int lda;
  bool ak;
  long long a_bytes;  // bytes from the base to the end of the last element, as b_bytes, c_bytes
  const float *B;  // B(k, n) = bk ? B[n * ldb + k] : B[k * ldb + n]
  int ldb;
  bool bk;
  long long b_bytes;
  const float *bias;
  bool bias_rows;
  const float *Cadd;
  int ldadd;
  float *C;
  int ldc;
  long long c_bytes;
  GemmCols cols;
  int M, N, K, relu;
  float *rs;  // rs[m] = sum_k A(m, k) from the same launch (needs !ak, !bk, unbatched C)
};

int gemm_run(const GemmProblem &q, void *workspace, hipStream_t s);
// split-K workspace bytes of an M x N x K product (any layout)
size_t gemm_ws(int M, int N, int K);

}  // namespace e2ep
