// The <threads, float4 vectors per thread> layout of the single-launch BatchNorm kernels
// (bn.hip k_bn_fwd_small / k_bn_bwd_small): one block per channel holds the channel's totv
// vectors in registers, thread t taking vectors t, t + T, ...  The fused MBConv middle
// (mbconv_mid.hip) repeats those kernels' summation order, so it takes its layout from here too.
#pragma once
#include "common.h"

namespace e2ep {

constexpr int BNS_T = 256, BNS_R = 8;  // at most BNS_R * BNS_T float4 (8192 elements) a channel

struct BnsLayout {
  int T, R;  // threads per block, vectors per thread; {0, 0}: the channel is too large
};

// 256-thread blocks of 1, 2, 4 or 8 vectors per thread.  e2ep_tune key 25 = 2: channels that
// need 8 per thread run 512-thread blocks of 4 instead (half the registers per thread, twice
// the waves per channel); key 26 = 2 does the same for the 2- and 4-vector cases.
inline BnsLayout bns_layout(int totv) {
  const int per = cdiv(totv, BNS_T);
  const bool lo = g_tune[TUNE_BNS_WIDE_LO] == 2, hi = g_tune[TUNE_BNS_WIDE] == 2;
  if (per <= 1) return {BNS_T, 1};
  if (per <= 2) return lo ? BnsLayout{2 * BNS_T, 1} : BnsLayout{BNS_T, 2};
  if (per <= 4) return lo ? BnsLayout{2 * BNS_T, 2} : BnsLayout{BNS_T, 4};
  if (per <= BNS_R) return hi ? BnsLayout{2 * BNS_T, 4} : BnsLayout{BNS_T, 8};
  return {0, 0};
}

}  // namespace e2ep
