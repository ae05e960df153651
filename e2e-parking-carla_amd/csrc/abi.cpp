// C-ABI bookkeeping shared by every kernel file: version + thread-local error message.
#include <stdarg.h>
#include <stdio.h>

#include "e2ep.h"
#include "tune.h"

namespace e2ep {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
// launch-plan tunables (tune.h TUNE_*), e2ep_tune.  Defaults from in-step A/B on the replayed
// C2 step (profiles/r02/session6/tune_ab_round*.txt): split-BN target 2048 (was 1024),
// depthwise weight-gradient target 1024 (was 2048), 1x1 weight-gradient target 1024 (was
// 2048) together -0.23 ms/step; the rest keep their values (no gain measured).  Round 6: split-BN
// target 8192 and 512 float4 per BN apply workgroup (was 2048 / 1024), C2 20.78 -> 20.58 ms
// (profiles/r06/bn_split_ab.txt); key 35 = 4, the direct-conv BEV stem forward and data
// gradient (mask 1 | 2) on 16-bit operands: C3 17.74 -> 17.53 ms (forward) -> 17.49 ms (data
// gradient).  On fp32 operands the forward (mask 16) took C2 20.56 -> 20.44 ms but moved the
// B = 8 eval-mode gradient-norm parity (test_model_b8_gpu) past its bound (1.36e-4 vs fp64 on
// one camera-encoder BN weight), and the fp32 data gradient (mask 8) alone is neutral, so fp32
// stays on the implicit GEMMs; the direct weight gradient (mask 4) is neutral in C3 and slower
// than k_conv_wgrad2 in fp32 (profiles/r06/stem_direct_ab.txt).  Key 36 = 2: the 16x16 MBConv
// middle in one launch per direction (mbconv_mid.hip; profiles/mbconv_mid/).  Key 37 = 2: the
// parameter-gradient finishing launches of a train step deferred to one batched launch per
// kind after the backward (pgrad.hip; profiles/pgrad_defer/).
int g_tune[TUNE_N] = {8192, 4096, 512, 512, 768, 1024, 512, 1, 1, 2, 1, 2, 2, 1, 2, 1, 1, 1, 1, 1, 1, 2, 1024, 2, 2048, 2, 1, 1, 2, 1, 2, 1, 1, 1, 1, 4, 2, 2};
}  // namespace e2ep

extern "C" {
int e2ep_abi_version(void) { return 4; }
int e2ep_tune(int key, int value) {
  if (key < 0 || key >= e2ep::TUNE_N || key == e2ep::TUNE_RETIRED_27 ||
      key == e2ep::TUNE_RETIRED_29 || key == e2ep::TUNE_RETIRED_31)
    return -1;
  const int prev = e2ep::g_tune[key];
  if (value > 0) e2ep::g_tune[key] = value;
  return prev;
}
const char *e2ep_last_error(void) { return e2ep::g_err; }
}
