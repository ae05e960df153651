// Internal interface of the attention kernels (attn.hip: vector-FMA kernels for every shape;
// attn_mf.hip: matrix-core kernels for the fusion encoder's long sequences).
#pragma once
#include <stdint.h>

#include "common.h"

namespace e2ep {

struct AttnDims {
  int B, H, Sq, Sk, dh;
  int q_ss, q_sb, kv_ss, kv_sb, o_ss, o_sb;  // element strides (sequence, batch)
  float scale, p;
  int causal;
};

enum AttnFamily {
  ATT_VEC,  // attn.hip: k_attn_fwd / k_attn_bwd_q / k_attn_bwd_kv / k_attn_w<DHP, ...>
  ATT_MF,   // attn_mf.hip: k_attn_fwd_mf / k_attn_bq_mf / k_attn_bkv_mf<NT>, k_attn_w_mf
};

// One pass's kernel and grid.
struct AttnPass {
  AttnFamily family;
  int dhp;    // ATT_VEC: head dim the kernel's registers hold, 44 (dh <= 44) or 64
  int lanes;  // ATT_VEC forward / dq: lanes per query, dk / dv: per key; 4 for sequences (of
              // queries, or keys for dk / dv) up to 16 (the control decoder's 14 tokens), else
              // e2ep_tune key 20 (1 automatic = 1, 2, 4: smaller tiles, more workgroups)
  int nt;     // ATT_MF: 128-wide tiles per wave along the staged sequence (Sk; Sq for dk / dv)
  dim3 grid;
};

// Which backward passes one `part` of e2ep_attn_bwd_part runs.
struct AttnBwdPart {
  bool d;            // D = dO . O into the workspace (k_attn_bwd_d)
  bool dq;
  bool dq_writes_d;  // dq's kernel, which computes D for its own rows in either family, also
                     // writes it to the workspace for dk / dv: part 0 runs no D pass
  bool dkv;          // reads D from the workspace
};

// Everything the host decides about one attention shape, decided once by attn_route() (attn.hip),
// the only reader of e2ep_tune keys 20 and 21.  The matrix-core family takes unmasked attention
// with Sq, Sk in {128, 256} and head dim <= 44 when key 21 >= 2: the forward, dq and the weights
// (2, default), and dk / dv too only with key 21 = 3 (the vector kernel is faster at that shape).
// Both families keep the same log2-domain lse, dropout counters and D = dO . O, so any forward
// pairs with any backward.
struct AttnRoute {
  AttnPass fwd, d, dq, dkv;
  AttnPass w[2];        // attention weights: [0] per head, [1] the head mean
  AttnBwdPart part[4];  // e2ep_attn_bwd_part's part: 0 all, 1 D only, 2 dq only, 3 dk / dv only
};
AttnRoute attn_route(const AttnDims &a, const uint8_t *key_pad);

// attn_mf.hip: launches of the ATT_MF passes
void attn_mf_fwd(const AttnPass &ps, const float *q, const float *k, const float *v,
                 const int *seed, const AttnDims &a, float *o, float *lse2, hipStream_t s);
// dq, and D into Dw when it is not null
void attn_mf_bq(const AttnPass &ps, const float *q, const float *k, const float *v, const float *o,
                const float *dout, const float *lse2, const int *seed, const AttnDims &a,
                float *dq, float *Dw, hipStream_t s);
void attn_mf_bkv(const AttnPass &ps, const float *q, const float *k, const float *v,
                 const float *dout, const float *lse2, const float *Dbuf, const int *seed,
                 const AttnDims &a, float *dk, float *dv, hipStream_t s);
// attention probabilities P = exp2(S - lse2): w [B][H][Sq][Sk], or the head mean [B][Sq][Sk]
// with average (heads summed in ascending order).  S is the forward kernel's own MFMA chain, so
// P is the matrix that forward normalised.
void attn_mf_weights(const AttnPass &ps, const float *q, const float *k, const float *lse2,
                     const AttnDims &a, int average, float *w, hipStream_t s);

}  // namespace e2ep
