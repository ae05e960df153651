// Deferred parameter-gradient finishing (pgrad.h): the deferral list and the batched kernels
// that e2ep_defer_flush launches, one per record kind, after the backward.
#include <mutex>
#include <vector>

#include "pgrad.h"

namespace e2ep {

// Records travel by value in the kernel arguments: a captured graph node keeps its arguments,
// so a replay needs no device table and the capture holds no host-to-device copy.  The batch
// sizes keep each argument block under 3 KB of the 4 KB a kernel may take; a flush with more
// records pending launches again with the remainder.
constexpr int SLAB_BATCH = 64;  // 40 B each
constexpr int LN_BATCH = 64;    // 32 B each
constexpr int SE_BATCH = 32;    // 80 B each

// first[j]: the first block of record j in the launch's grid; first[count]: the grid size.
template <typename Rec, int MAX>
struct Batch {
  Rec r[MAX];
  int first[MAX + 1];
  int count;
};

// The record whose block range holds block b (uniform over the block: scalar loads of the
// kernel arguments, log2(MAX) steps).
template <typename Rec, int MAX>
__device__ __forceinline__ int batch_find(const Batch<Rec, MAX> &t, int b) {
  int lo = 0, hi = t.count;  // first[lo] <= b < first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.first[mid] <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Both flavours of the slab sum in 1024-thread blocks: a 16-lane record's block is a
// k_reduce_splits block; a float4 record's block covers four consecutive k_reduce_splits4
// blocks (its threads are independent, one per 4 outputs).
__global__ void __launch_bounds__(1024) k_reduce_splits_batch(const Batch<SlabRec, SLAB_BATCH> t) {
  __shared__ float red[16][64];
  const int j = batch_find(t, (int)blockIdx.x);
  const SlabRec &r = t.r[j];
  const int blk = (int)blockIdx.x - t.first[j];
  if (r.flags & 2) {
    const int i = (blk * 1024 + (int)threadIdx.x) * 4;
    if (i < r.n) reduce_splits4_thread(r.part, r.splits, r.n, r.out, r.flags & 1, r.RS, r.mask, i);
  } else {
    reduce_splits_block(r.part, r.splits, r.n, r.out, r.flags & 1, r.RS, r.mask, blk, red);
  }
}

// Block (bx, by) of k_ln_param_grads' grid (E / 64, 2) is block by * (E / 64) + bx of its record.
__global__ void __launch_bounds__(1024) k_ln_param_grads_batch(const Batch<LnRec, LN_BATCH> t) {
  __shared__ float red[16][64];
  const int j = batch_find(t, (int)blockIdx.x);
  const LnRec &r = t.r[j];
  const int blk = (int)blockIdx.x - t.first[j], gx = (r.E + 63) / 64;
  ln_param_grads_block(r.part, r.nblk, r.E, r.dgamma, r.dbeta, blk % gx, blk / gx, red);
}

__global__ void __launch_bounds__(256) k_se_wgrad_batch(const Batch<SeRec, SE_BATCH> t) {
  const int j = batch_find(t, (int)blockIdx.x);
  const SeRec &r = t.r[j];
  const int blk = (int)blockIdx.x - t.first[j];
  se_wgrad_thread(r.pooled, r.hpre, r.da, r.dhpre, r.N, r.C, r.sq, r.dw1, r.db1, r.dw2, r.db2,
                  blk * 256 + (int)threadIdx.x);
}

// Process-global, not thread_local: autograd runs the backward nodes (the call sites) on its own
// thread while the scope is opened and flushed from the caller's thread.  Those accesses are
// sequential; the mutex only makes a misuse from two threads at once harmless.
static std::mutex g_mu;
static bool g_open = false;
static int g_hold = 0;
static std::vector<SlabRec> g_slabs;
static std::vector<LnRec> g_lns;
static std::vector<SeRec> g_ses;

// key 37: 1 = launch immediately, 2 = defer every kind, 3 = defer the conv slabs only (A/B)
static bool defer_on(bool slabs) {
  const int v = g_tune[TUNE_PGRAD_DEFER];
  return g_open && !g_hold && (v == 2 || (v == 3 && slabs));
}

bool pgrad_defer(const SlabRec &r) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!defer_on(true)) return false;
  g_slabs.push_back(r);
  return true;
}
bool pgrad_defer(const LnRec &r) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!defer_on(false)) return false;
  g_lns.push_back(r);
  return true;
}
bool pgrad_defer(const SeRec &r) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!defer_on(false)) return false;
  g_ses.push_back(r);
  return true;
}

static int blocks_of(const SlabRec &r) {
  return (r.flags & 2) ? cdiv(r.n / 4, 1024) : cdiv(r.n, 64);
}
static int blocks_of(const LnRec &r) { return cdiv(r.E, 64) * 2; }
static int blocks_of(const SeRec &r) { return cdiv(2 * r.sq * r.C + r.sq + r.C, 256); }

// A launch must not hold two slab records of one output: an accumulating record reads what the
// earlier one writes.  Such a record starts the next launch, which the stream orders after
// this one.  (The LayerNorm and SE kinds have no accumulate mode: a parameter used twice in a
// backward is the caller's to send down the immediate path, as e2ep.h says.)
static bool repeats(const SlabRec *r, int have) {
  for (int k = 0; k < have; ++k)
    if (r[k].out == r[have].out) return true;
  return false;
}
static bool repeats(const LnRec *, int) { return false; }
static bool repeats(const SeRec *, int) { return false; }

template <typename Rec, int MAX, typename K>
static void flush_kind(const std::vector<Rec> &recs, K kernel, int threads, hipStream_t s) {
  size_t at = 0;
  while (at < recs.size()) {
    Batch<Rec, MAX> t;
    int c = 0, blocks = 0;
    for (; c < MAX && at + c < recs.size() && !(c > 0 && repeats(&recs[at], c)); ++c) {
      t.r[c] = recs[at + c];
      t.first[c] = blocks;
      blocks += blocks_of(t.r[c]);
    }
    for (int k = c; k <= MAX; ++k) t.first[k] = blocks;
    for (int k = c; k < MAX; ++k) t.r[k] = Rec{};
    t.count = c;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, s, t);
    at += c;
  }
}

}  // namespace e2ep

using namespace e2ep;

extern "C" {

int e2ep_defer_begin(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  E2EP_REQUIRE(!g_open, E2EP_EINVAL, "e2ep_defer_begin: a deferral scope is already open");
  g_open = true;
  g_hold = 0;
  return 0;
}

int e2ep_defer_flush(void *stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  E2EP_REQUIRE(g_open, E2EP_EINVAL, "e2ep_defer_flush: no deferral scope is open");
  hipStream_t s = as_stream(stream);
  flush_kind<SlabRec, SLAB_BATCH>(g_slabs, k_reduce_splits_batch, 1024, s);
  flush_kind<LnRec, LN_BATCH>(g_lns, k_ln_param_grads_batch, 1024, s);
  flush_kind<SeRec, SE_BATCH>(g_ses, k_se_wgrad_batch, 256, s);
  g_slabs.clear();
  g_lns.clear();
  g_ses.clear();
  g_open = false;
  g_hold = 0;
  return launch_status("e2ep_defer_flush");
}

int e2ep_defer_abort(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_slabs.clear();
  g_lns.clear();
  g_ses.clear();
  g_open = false;
  g_hold = 0;
  return 0;
}

int e2ep_defer_pending(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  return (int)(g_slabs.size() + g_lns.size() + g_ses.size());
}

int e2ep_defer_hold(int hold) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int prev = g_hold;
  g_hold = hold ? 1 : 0;
  return prev;
}

}  // extern "C"
