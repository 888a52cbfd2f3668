// kernels.hip — MI355X (gfx950/CDNA4) kernels + C-ABI host layer of
// libballista_gpu.so, the GPU stage executor behind Ballista's
// ExecutionEngine seam (see include/ballista_gpu.h for the ABI contract and
// per-entry-point reference citations).
//
// Design notes (MI355X-first; /opt/skills/guides/cdna_hip_programming.md):
//  - Everything here is HBM-bound integer/byte work (scan, compare, hash,
//    split, gather, 128-bit accumulate) — no dense contraction, no MFMA.
//  - wave64 is the unit: selection masks are built with 64-bit __ballot
//    (Arrow LSB bitmap order == ballot lane order), stable compaction and
//    the stable multi-split use wave-contiguous row chunks so row order is
//    preserved without cross-wave coordination.
//  - Loads are coalesced full-width: Decimal128 as ulong2 (16 B/lane),
//    Date32 as i32 (256 B/wave).  Grid-stride loops capped at ~2048 blocks
//    (guide §6 G11).
//  - Exact Decimal128 arithmetic: two's-complement i128 adds/muls are
//    wrap-exact and associative, so block/wave reduction order never changes
//    the result; global accumulation uses the u64 carry-propagating
//    atomicAdd pair (deterministic, order-independent).
//  - Grouped aggregation clusters the wave's rows by group with ballot
//    leader-loops (few distinct groups per wave in the TPC-H shapes), does
//    register wave-reductions, and lands ONE LDS atomic set per
//    (group, wave-iteration) instead of per row.

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/ballista_gpu.h"
#include "bg_ahash.h"
#include "bg_internal.h"

#define BG_BLOCK 256
#define BG_MAX_BLOCKS 2048
#define BG_WAVE 64
#define BG_MAX_PREDS 8
#define BG_MAX_KEYS 4
#define BG_MAX_PAYLOAD 16

static inline int64_t bg_imin64(int64_t a, int64_t b) { return a < b ? a : b; }

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static thread_local bool g_inited = false;

static thread_local double g_last_kernel_ms = 0.0;

extern "C" const char* bg_last_error(void) { return g_err; }
extern "C" int bg_version(void) { return 12; }

// Build provenance: the sha256 over the library's seven sources
// (kernels.hip, bg_ahash.h, stage.cpp, stage_ipc.h, stage_json.h,
// stage_parquet.h, ballista_gpu.h) injected by __graft_entry__.build(); a
// CPU test
// recomputes the hash over the committed sources and fails when the
// committed .so was not built from them.
#ifndef BG_SOURCE_HASH
#define BG_SOURCE_HASH "unverified-local-build"
#endif
extern "C" const char* bg_source_hash(void) { return BG_SOURCE_HASH; }

// Duration of the most recent timed hot kernel (bg_q6_agg / bg_q1_agg),
// measured with hipEvents on the launch stream — feeds bench.py's
// roofline.achieved (algorithmic bytes / kernel time).
extern "C" double bg_last_kernel_ms(void) { return g_last_kernel_ms; }

static int set_err(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}

static int set_hip_err(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return BG_ERR_HIP;
}

#define HIP_TRY(call)                                   \
  do {                                                  \
    hipError_t _e = (call);                             \
    if (_e != hipSuccess) return set_hip_err(_e, #call); \
  } while (0)

// ---------------------------------------------------------------------------
// pooled device allocator — hipMalloc/hipFree cost ~100 ms on GB-scale
// temporaries (measured: join-probe pair buffers), so every internal
// allocation (and the public bg_malloc/bg_free) goes through a size-bucketed
// free list (power-of-two rounding, per-process, mutex-guarded).  Sized for
// 288 GB HBM: memory stays pooled until bg_pool_trim().
// ---------------------------------------------------------------------------
static std::mutex g_pool_mu;
static std::unordered_map<uint64_t, std::vector<void*>> g_pool_free;
static std::unordered_map<void*, uint64_t> g_pool_sizes;
static std::set<void*> g_pool_freeset;
// accounting for bg_pool_stats(), kept under g_pool_mu: buffers handed out
// and not yet released ("live"), and bytes parked in the free lists
static int64_t g_pool_live_bytes = 0;
static int64_t g_pool_live_buffers = 0;
static int64_t g_pool_cached_bytes = 0;

static uint64_t pool_round(uint64_t bytes) {
  uint64_t p = 256;
  while (p < bytes) p <<= 1;
  return p;
}

static hipError_t pool_malloc(void** out, uint64_t bytes) {
  const uint64_t sz = pool_round(bytes ? bytes : 1);
  {
    std::lock_guard<std::mutex> g(g_pool_mu);
    auto it = g_pool_free.find(sz);
    if (it != g_pool_free.end() && !it->second.empty()) {
      *out = it->second.back();
      it->second.pop_back();
      g_pool_freeset.erase(*out);
      g_pool_cached_bytes -= (int64_t)sz;
      g_pool_live_bytes += (int64_t)sz;
      ++g_pool_live_buffers;
      return hipSuccess;
    }
  }
  hipError_t e = hipMalloc(out, sz);
  if (e != hipSuccess) {  // pressure: drop the cache and retry once
    std::lock_guard<std::mutex> g(g_pool_mu);
    for (auto& kv : g_pool_free)
      for (void* p : kv.second) {
        g_pool_sizes.erase(p);
        (void)hipFree(p);
      }
    g_pool_free.clear();
    g_pool_freeset.clear();
    g_pool_cached_bytes = 0;
    e = hipMalloc(out, sz);
  }
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> g(g_pool_mu);
    g_pool_sizes[*out] = sz;
    g_pool_live_bytes += (int64_t)sz;
    ++g_pool_live_buffers;
  }
  return e;
}

static hipError_t pool_release(void* p) {
  if (!p) return hipSuccess;
  std::lock_guard<std::mutex> g(g_pool_mu);
  auto it = g_pool_sizes.find(p);
  if (it == g_pool_sizes.end()) return hipFree(p);  // not pooled
  // double-release guard: handing one buffer to two later allocations
  // aliases them and corrupts unrelated state — fail loudly instead
  if (!g_pool_freeset.insert(p).second) {
    fprintf(stderr, "bg pool: DOUBLE RELEASE of %p (size %llu)\n", p,
            (unsigned long long)it->second);
    abort();
  }
  g_pool_free[it->second].push_back(p);
  g_pool_live_bytes -= (int64_t)it->second;
  --g_pool_live_buffers;
  g_pool_cached_bytes += (int64_t)it->second;
  return hipSuccess;
}

extern "C" int bg_pool_trim(void) {
  std::lock_guard<std::mutex> g(g_pool_mu);
  for (auto& kv : g_pool_free)
    for (void* p : kv.second) {
      g_pool_sizes.erase(p);
      (void)hipFree(p);
    }
  g_pool_free.clear();
  g_pool_freeset.clear();
  g_pool_cached_bytes = 0;
  return BG_OK;
}

extern "C" int bg_pool_stats(int64_t* live_bytes, int64_t* live_buffers,
                             int64_t* cached_bytes) {
  std::lock_guard<std::mutex> g(g_pool_mu);
  if (live_bytes) *live_bytes = g_pool_live_bytes;
  if (live_buffers) *live_buffers = g_pool_live_buffers;
  if (cached_bytes) *cached_bytes = g_pool_cached_bytes;
  return BG_OK;
}

// Scoped owner of one pooled device buffer: released when it goes out of
// scope, so every return path of a host wrapper (HIP_TRY included) gives
// its temporaries back.  Releasing at scope exit, with kernels that read
// the buffer possibly still in flight, is safe because ALL library work is
// issued on the one legacy null stream (every launch and every async
// memset/copy in this file passes stream 0, bg_q6_agg included, the
// blocking hipMemcpy/hipMemset calls use it implicitly, and no other
// stream is ever created): whoever takes the buffer from the pool next can
// only touch it with work that the stream orders after its previous user.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p;
      o.p = nullptr;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  // count == 0 still allocates one element: callers pass the pointer on
  hipError_t alloc(int64_t count) {
    reset();
    void* q = nullptr;
    hipError_t e = pool_malloc(&q, sizeof(T) * (uint64_t)(count ? count : 1));
    if (e == hipSuccess) p = (T*)q;
    return e;
  }
  void reset() {
    if (p) (void)pool_release(p);
    p = nullptr;
  }
  // hand the pointer to a longer-lived owner (join handles)
  T* detach() {
    T* q = p;
    p = nullptr;
    return q;
  }
  void swap(DevBuf& o) { std::swap(p, o.p); }
  T* get() const { return p; }
  operator T*() const { return p; }
};

// Scoped pair of timing events (create-per-call, destroyed on every path).
struct EventPair {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  ~EventPair() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
  hipError_t create() {
    hipError_t e = hipEventCreate(&ev0);
    return e != hipSuccess ? e : hipEventCreate(&ev1);
  }
};

// grid size for `items` work items at `per_block` items per block:
// ceil(items / per_block), capped at BG_MAX_BLOCKS, never 0
static inline int grid_for(int64_t items, int64_t per_block = BG_BLOCK) {
  const int64_t b = bg_imin64((items + per_block - 1) / per_block,
                              BG_MAX_BLOCKS);
  return b < 1 ? 1 : (int)b;
}

// The shared body of the bg_*_batch wrappers: upload `njobs` host job
// records, zero an int error flag, launch kernel(jobs, njobs, extra...,
// flag) on `blocks` blocks and read the flag back into *err_out.  The
// caller keeps its own grid rule and its own flag -> error mapping.
template <typename Job, typename Kernel, typename... Extra>
static int run_job_batch(Kernel kernel, const Job* h_jobs, int64_t njobs,
                         int blocks, int* err_out, Extra... extra) {
  DevBuf<Job> d_jobs;
  DevBuf<int> d_err;
  HIP_TRY(d_jobs.alloc(njobs));
  HIP_TRY(d_err.alloc(1));
  HIP_TRY(hipMemset(d_err, 0, sizeof(int)));
  HIP_TRY(hipMemcpy(d_jobs, h_jobs, sizeof(Job) * njobs,
                    hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(BG_BLOCK), 0, 0, d_jobs.get(),
                     njobs, extra..., d_err.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(err_out, d_err, sizeof(int), hipMemcpyDeviceToHost));
  return BG_OK;
}

#define REQUIRE_INIT()                                                       \
  do {                                                                       \
    if (!g_inited)                                                           \
      return set_err(BG_ERR_NO_GPU,                                          \
                     "ballista_gpu: bg_init() not called or no gfx950 GPU "  \
                     "present — the GPU stage executor has NO CPU fallback"); \
  } while (0)

// ---------------------------------------------------------------------------
// session
// ---------------------------------------------------------------------------
extern "C" int bg_init(int device_ordinal) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return set_err(BG_ERR_NO_GPU, "ballista_gpu: no HIP device visible");
  HIP_TRY(hipSetDevice(device_ordinal));
  // touch the device so a broken runtime fails here, loudly
  HIP_TRY(hipFree(nullptr));
  g_inited = true;
  return BG_OK;
}

extern "C" int bg_device_count(int* out) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  *out = n;
  return BG_OK;
}

extern "C" int bg_synchronize(void) {
  REQUIRE_INIT();
  HIP_TRY(hipDeviceSynchronize());
  return BG_OK;
}

extern "C" int bg_malloc(uint64_t bytes, void** d_ptr) {
  REQUIRE_INIT();
  HIP_TRY(pool_malloc((void**)d_ptr, bytes));
  return BG_OK;
}
extern "C" int bg_free(void* d_ptr) {
  REQUIRE_INIT();
  HIP_TRY(pool_release(d_ptr));
  return BG_OK;
}
extern "C" int bg_memset(void* d_ptr, int value, uint64_t bytes) {
  REQUIRE_INIT();
  HIP_TRY(hipMemset(d_ptr, value, bytes));
  return BG_OK;
}
extern "C" int bg_memcpy_h2d(void* d_dst, const void* h_src, uint64_t bytes) {
  REQUIRE_INIT();
  HIP_TRY(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
  return BG_OK;
}
extern "C" int bg_memcpy_d2h(void* h_dst, const void* d_src, uint64_t bytes) {
  REQUIRE_INIT();
  HIP_TRY(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
  return BG_OK;
}
extern "C" int bg_memcpy_dtod(void* d_dst, const void* d_src, uint64_t bytes) {
  REQUIRE_INIT();
  HIP_TRY(hipMemcpy(d_dst, d_src, bytes, hipMemcpyDeviceToDevice));
  return BG_OK;
}

// ---------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------
using u64 = unsigned long long;
using i64 = long long;
using u128 = unsigned __int128;
using i128 = __int128;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (BG_WAVE - 1); }

__device__ __forceinline__ bool bit_valid(const uint8_t* bm, int64_t i) {
  return bm == nullptr || ((bm[i >> 3] >> (i & 7)) & 1);
}

__device__ __forceinline__ i128 make_i128(u64 lo, i64 hi) {
  return ((i128)hi << 64) | (i128)(u128)lo;
}

__device__ __forceinline__ i128 load_dec128(const void* base, int64_t row) {
  const ulong2 v = reinterpret_cast<const ulong2*>(base)[row];
  return make_i128(v.x, (i64)v.y);
}

// order-independent exact i128 accumulate into a global (lo, hi) pair
__device__ __forceinline__ void atomic_add_i128(u64* lo, u64* hi, i128 v) {
  u64 vlo = (u64)(u128)v;
  u64 vhi = (u64)((u128)v >> 64);
  u64 old = atomicAdd(lo, vlo);
  u64 carry = (old + vlo) < vlo ? 1ull : 0ull;
  if (vhi + carry) atomicAdd(hi, vhi + carry);
}

// full-wave i128 sum (all 64 lanes get the total)
__device__ __forceinline__ i128 wave_reduce_i128(i128 v) {
  u64 lo = (u64)(u128)v;
  u64 hi = (u64)((u128)v >> 64);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    u64 olo = (u64)__shfl_xor((long long)lo, s, BG_WAVE);
    u64 ohi = (u64)__shfl_xor((long long)hi, s, BG_WAVE);
    u64 nlo = lo + olo;
    hi = hi + ohi + (nlo < olo ? 1 : 0);
    lo = nlo;
  }
  return make_i128(lo, (i64)hi);
}

// ---------------------------------------------------------------------------
// predicate evaluation -> Arrow LSB bitmask
// ---------------------------------------------------------------------------
struct PredDev {
  const void* data;
  const uint8_t* valid;
  int dtype;
  int op;
  u64 lo_lo; i64 lo_hi;
  u64 hi_lo; i64 hi_hi;
};

struct PredArgs {
  int npreds;
  PredDev p[BG_MAX_PREDS];
};

__device__ __forceinline__ bool pred_eval(i128 x, int op, i128 lo, i128 hi) {
  switch (op) {
    case BG_PRED_GE_LT: return x >= lo && x < hi;
    case BG_PRED_BETWEEN: return x >= lo && x <= hi;
    case BG_PRED_LT: return x < hi;
    case BG_PRED_EQ: return x == lo;
    case BG_PRED_GT: return x > lo;
    default: return false;
  }
}

// one wave evaluates 64 consecutive rows per step; ballot bit order ==
// Arrow LSB bitmap order, lane 0 stores the u64 word.
__global__ void k_eval_predicates(PredArgs args, int64_t n, u64* mask_words,
                                  int64_t nwords) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t w = wave_global; w < nwords; w += nwaves) {
    const int64_t row = w * BG_WAVE + lane_id();
    bool keep = row < n;
    if (keep) {
      for (int pi = 0; pi < args.npreds; ++pi) {
        const PredDev& pr = args.p[pi];
        if (!bit_valid(pr.valid, row)) { keep = false; break; }
        i128 x;
        switch (pr.dtype) {
          case BG_DT_INT32:
          case BG_DT_DATE32:
            x = (i128)__builtin_nontemporal_load(
                reinterpret_cast<const int32_t*>(pr.data) + row);
            break;
          case BG_DT_INT64:
            x = (i128)__builtin_nontemporal_load(
                reinterpret_cast<const int64_t*>(pr.data) + row);
            break;
          case BG_DT_DECIMAL128: {
            typedef unsigned long long ull2_ev
                __attribute__((ext_vector_type(2)));
            const ull2_ev v = __builtin_nontemporal_load(
                reinterpret_cast<const ull2_ev*>(pr.data) + row);
            x = make_i128(v[0], (i64)v[1]);
            break;
          }
          case BG_DT_DICT8:
            x = (i128) reinterpret_cast<const uint8_t*>(pr.data)[row];
            break;
          case BG_DT_FLOAT64: {
            // float predicates compare in f64 (bounds arrive as f64 BITS in
            // lo_lo/hi_lo); comparisons with NaN are false, matching SQL
            const double xv = reinterpret_cast<const double*>(pr.data)[row];
            double flo, fhi;
            __builtin_memcpy(&flo, &pr.lo_lo, 8);
            __builtin_memcpy(&fhi, &pr.hi_lo, 8);
            bool kp;
            switch (pr.op) {
              case BG_PRED_GE_LT: kp = xv >= flo && xv < fhi; break;
              case BG_PRED_BETWEEN: kp = xv >= flo && xv <= fhi; break;
              case BG_PRED_LT: kp = xv < fhi; break;
              case BG_PRED_EQ: kp = xv == flo; break;
              case BG_PRED_GT: kp = xv > flo; break;
              default: kp = false;
            }
            if (!kp) keep = false;
            x = 0;
            break;
          }
          default:
            x = 0;
        }
        if (!keep) break;      // a failed float predicate short-circuits
        if (pr.dtype == BG_DT_FLOAT64) continue;  // handled above
        if (!pred_eval(x, pr.op, make_i128(pr.lo_lo, pr.lo_hi),
                       make_i128(pr.hi_lo, pr.hi_hi))) {
          keep = false;
          break;
        }
      }
    }
    u64 m = __ballot(keep);
    if (lane_id() == 0) mask_words[w] = m;
  }
}

extern "C" int bg_eval_predicates(const bg_column* cols, int32_t ncols,
                                  const bg_pred* preds, int32_t npreds,
                                  int64_t n, uint8_t* d_mask) {
  REQUIRE_INIT();
  if (npreds <= 0 || npreds > BG_MAX_PREDS)
    return set_err(BG_ERR_INVALID, "npreds out of range [1,8]");
  PredArgs a{};
  a.npreds = npreds;
  for (int i = 0; i < npreds; ++i) {
    int c = preds[i].column;
    if (c < 0 || c >= ncols) return set_err(BG_ERR_INVALID, "pred column oob");
    a.p[i].data = cols[c].d_data;
    a.p[i].valid = cols[c].d_validity;
    a.p[i].dtype = cols[c].dtype;
    a.p[i].op = preds[i].op;
    a.p[i].lo_lo = (u64)preds[i].lo_lo;
    a.p[i].lo_hi = preds[i].lo_hi;
    a.p[i].hi_lo = (u64)preds[i].hi_lo;
    a.p[i].hi_hi = preds[i].hi_hi;
  }
  int64_t nwords = (n + 63) / 64;
  int blocks = grid_for(nwords * BG_WAVE);
  hipLaunchKernelGGL(k_eval_predicates, dim3(blocks), dim3(BG_BLOCK), 0, 0, a,
                     n, reinterpret_cast<u64*>(d_mask), nwords);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---------------------------------------------------------------------------
// generic exclusive scan (single block; m up to a few million)
// used for compaction offsets and the multi-split histogram
// ---------------------------------------------------------------------------
// Segment-aware exclusive scan: block b owns [b*seg, min((b+1)*seg, m));
// seg_bases (optional) gives each block's running base.  With gridDim.x == 1
// and seg >= m this is the whole-array scan (small inputs).
template <typename IN>
__global__ void k_exclusive_scan_i64(const IN* in, int64_t m, i64* out,
                                     i64* total, int64_t seg,
                                     const i64* seg_bases) {
  __shared__ i64 sums[BG_BLOCK];
  __shared__ i64 carry;
  const int64_t seg_lo = (int64_t)blockIdx.x * seg;
  const int64_t seg_hi = min(seg_lo + seg, m);
  if (seg_lo >= m) return;
  const int t = threadIdx.x;
  const int64_t len = seg_hi - seg_lo;
  const int64_t ch = (len + blockDim.x - 1) / blockDim.x;
  const int64_t lo = seg_lo + (int64_t)t * ch;
  const int64_t hi = min(lo + ch, seg_hi);
  i64 s = 0;
  for (int64_t i = lo; i < hi; ++i) s += (i64)in[i];
  sums[t] = s;
  __syncthreads();
  if (t == 0) {
    i64 acc = seg_bases ? seg_bases[blockIdx.x] : 0;
    for (int i = 0; i < (int)blockDim.x; ++i) {
      i64 v = sums[i];
      sums[i] = acc;
      acc += v;
    }
    carry = acc;
  }
  __syncthreads();
  i64 acc = sums[t];
  for (int64_t i = lo; i < hi; ++i) {
    i64 v = (i64)in[i];
    out[i] = acc;
    acc += v;
  }
  if (t == 0 && total && seg_hi == m) *total = carry;
}

// per-segment sums for the hierarchical scan's first phase
template <typename IN>
__global__ void k_segment_sums_i64(const IN* in, int64_t m, int64_t seg,
                                   u64* seg_sums, int64_t nseg) {
  __shared__ i64 sums[BG_BLOCK];
  for (int64_t b = blockIdx.x; b < nseg; b += gridDim.x) {
    const int64_t lo = b * seg, hi = min(lo + seg, m);
    i64 s = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
      s += (i64)in[i];
    sums[threadIdx.x] = s;
    __syncthreads();
    for (int st = blockDim.x / 2; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) sums[threadIdx.x] += sums[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) seg_sums[b] = (u64)sums[0];
    __syncthreads();
  }
}

// Host-side hierarchical exclusive scan (two levels; m up to ~10^9).
// ---------------------------------------------------------------------------
// Single-pass exclusive scan (decoupled lookback): tiles are acquired in
// order through a ticket counter (so every predecessor of a spinning tile
// is resident and progressing — deadlock-free), each tile publishes
// {flag, value} packed in ONE u64 (flag in bits 63:62: 1 = aggregate,
// 2 = inclusive prefix; values must stay < 2^62 — counts/byte-lengths do),
// with agent-scope release/acquire atomics (MI355X XCDs have private L2s;
// scope-agent makes the handoff visible across them).  16 B/element of
// traffic vs the 3-pass hierarchical scan's 24, and one launch instead of
// three.
// ---------------------------------------------------------------------------
#define SCAN_TILE 4096
#define SCAN_ELEMS (SCAN_TILE / BG_BLOCK)
#define SCAN_FLAG_SHIFT 62

__global__ void k_scan_lookback(const u64* in, int64_t n, i64* out,
                                i64* total_out, u64* state, int* ticket,
                                int64_t ntiles) {
  __shared__ u64 lds[SCAN_TILE];
  __shared__ u64 tsum[BG_BLOCK];
  __shared__ u64 texcl[BG_BLOCK];
  __shared__ u64 s_carry;
  __shared__ int s_tile;
  const int tid = threadIdx.x;
  while (true) {
    if (tid == 0) s_tile = atomicAdd(ticket, 1);
    __syncthreads();
    const int64_t tile = s_tile;
    if (tile >= ntiles) return;
    const int64_t base = tile * SCAN_TILE;
    const int64_t lim = n - base < SCAN_TILE ? n - base : SCAN_TILE;
    for (int i = tid; i < SCAN_TILE; i += BG_BLOCK)
      lds[i] = (i < lim) ? __builtin_nontemporal_load(&in[base + i]) : 0;
    __syncthreads();
    u64 run = 0;
    for (int j = 0; j < SCAN_ELEMS; ++j) {
      const int i = tid * SCAN_ELEMS + j;
      const u64 v = lds[i];
      lds[i] = run;  // exclusive within this thread's chunk
      run += v;
    }
    tsum[tid] = run;
    __syncthreads();
    for (int off = 1; off < BG_BLOCK; off <<= 1) {
      const u64 v = (tid >= off) ? tsum[tid - off] : 0;
      __syncthreads();
      tsum[tid] += v;
      __syncthreads();
    }
    const u64 agg = tsum[BG_BLOCK - 1];
    texcl[tid] = (tid == 0) ? 0 : tsum[tid - 1];
    if (tid == 0) {
      if (tile == 0) {
        __hip_atomic_store(&state[0], agg | (2ull << SCAN_FLAG_SHIFT),
                           __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        s_carry = 0;
      } else {
        __hip_atomic_store(&state[tile], agg | (1ull << SCAN_FLAG_SHIFT),
                           __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        u64 carry = 0;
        int64_t t = tile - 1;
        while (t >= 0) {
          u64 st;
          do {
            st = __hip_atomic_load(&state[t], __ATOMIC_ACQUIRE,
                                   __HIP_MEMORY_SCOPE_AGENT);
            if (!(st >> SCAN_FLAG_SHIFT)) __builtin_amdgcn_s_sleep(2);
          } while (!(st >> SCAN_FLAG_SHIFT));
          carry += st & ((1ull << SCAN_FLAG_SHIFT) - 1);
          if ((st >> SCAN_FLAG_SHIFT) == 2ull) break;
          --t;
        }
        __hip_atomic_store(&state[tile],
                           (carry + agg) | (2ull << SCAN_FLAG_SHIFT),
                           __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        s_carry = carry;
      }
      if (tile == ntiles - 1 && total_out) *total_out = (i64)(s_carry + agg);
    }
    __syncthreads();
    const u64 carry = s_carry;
    for (int i = tid; i < lim; i += BG_BLOCK)
      out[base + i] = (i64)(carry + texcl[i / SCAN_ELEMS] + lds[i]);
    __syncthreads();
  }
}

template <typename IN>
static int scan_exclusive_t(const IN* d_in, int64_t m, i64* d_out,
                            i64* d_total) {
  if (m <= 0) {
    // nothing to scan: the total must still be DEFINED (pool buffers are
    // recycled — stale bytes here once leaked a phantom match count)
    if (d_total) {
      hipError_t e = hipMemsetAsync(d_total, 0, sizeof(i64), 0);
      if (e != hipSuccess) return set_hip_err(e, "scan total zero");
    }
    return BG_OK;
  }
  const int64_t SMALL = 1 << 18;
  if (m <= SMALL) {
    hipLaunchKernelGGL(k_exclusive_scan_i64, dim3(1), dim3(BG_BLOCK), 0, 0,
                       d_in, m, d_out, d_total, m > 0 ? m : 1, nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_hip_err(e, "scan small");
    return BG_OK;
  }
  // single-pass decoupled-lookback scan: MEASURED NEGATIVE on MI355X
  // (31.6 ms vs 12.4 ms hierarchical at 322M elements — the ticket +
  // LDS block-scan + spin overhead at 4096-element tiles outweighs the
  // 24->16 B/element traffic saving).  Kept behind BG_SCAN_LOOKBACK=1.
  const char* envs = getenv("BG_SCAN_LOOKBACK");
  if (sizeof(IN) == 8 && envs && envs[0] == '1') {
    const int64_t ntiles = (m + SCAN_TILE - 1) / SCAN_TILE;
    DevBuf<u64> d_state;
    DevBuf<int> d_ticket;
    hipError_t e;
    e = d_state.alloc(ntiles);
    if (e != hipSuccess) return set_hip_err(e, "scan malloc");
    e = d_ticket.alloc(1);
    if (e != hipSuccess) return set_hip_err(e, "scan malloc");
    e = hipMemsetAsync(d_state, 0, sizeof(u64) * ntiles, 0);
    if (e != hipSuccess) return set_hip_err(e, "scan memset");
    e = hipMemsetAsync(d_ticket, 0, sizeof(int), 0);
    if (e != hipSuccess) return set_hip_err(e, "scan memset");
    int blocks = (int)bg_imin64(ntiles, BG_MAX_BLOCKS);
    hipLaunchKernelGGL(k_scan_lookback, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                       (const u64*)(const void*)d_in, m, d_out, d_total,
                       d_state, d_ticket, ntiles);
    e = hipGetLastError();
    if (e != hipSuccess) return set_hip_err(e, "scan lookback");
    return BG_OK;
  }
  const int64_t seg = 1 << 16;  // 65536 elems per block segment
  const int64_t nseg = (m + seg - 1) / seg;
  DevBuf<u64> d_segsums;
  DevBuf<i64> d_segbases;
  hipError_t e;
  e = d_segsums.alloc(nseg);
  if (e != hipSuccess) return set_hip_err(e, "scan malloc");
  e = d_segbases.alloc(nseg);
  if (e != hipSuccess) return set_hip_err(e, "scan malloc");
  int blocks = (int)bg_imin64(nseg, BG_MAX_BLOCKS);
  hipLaunchKernelGGL(k_segment_sums_i64, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     d_in, m, seg, d_segsums, nseg);
  hipLaunchKernelGGL(k_exclusive_scan_i64, dim3(1), dim3(BG_BLOCK), 0, 0,
                     d_segsums.get(), nseg, d_segbases.get(), d_total, nseg,
                     nullptr);
  hipLaunchKernelGGL(k_exclusive_scan_i64, dim3((uint32_t)nseg),
                     dim3(BG_BLOCK), 0, 0, d_in, m, d_out, nullptr, seg,
                     d_segbases);
  e = hipGetLastError();
  if (e != hipSuccess) return set_hip_err(e, "scan large");
  return BG_OK;
}

static int scan_exclusive_i64(const u64* d_in, int64_t m, i64* d_out,
                              i64* d_total) {
  return scan_exclusive_t<u64>(d_in, m, d_out, d_total);
}

static int scan_exclusive_u32(const uint32_t* d_in, int64_t m, i64* d_out,
                              i64* d_total) {
  return scan_exclusive_t<uint32_t>(d_in, m, d_out, d_total);
}


// ---------------------------------------------------------------------------
// stable mask compaction
// ---------------------------------------------------------------------------
#define MC_WORDS_PER_WAVE 1024  // 65536 rows per wave chunk

__global__ void k_mask_count(const u64* words, int64_t nwords, int64_t n,
                             u64* wave_counts, int64_t nchunks) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t c = wave_global; c < nchunks; c += nwaves) {
    const int64_t w0 = c * MC_WORDS_PER_WAVE;
    const int64_t w1 = min(w0 + (int64_t)MC_WORDS_PER_WAVE, nwords);
    u64 cnt = 0;
    for (int64_t w = w0 + lane_id(); w < w1; w += BG_WAVE) {
      u64 m = words[w];
      // trim tail bits beyond n in the last word
      if (w == nwords - 1 && (n & 63)) m &= (1ull << (n & 63)) - 1;
      cnt += __popcll(m);
    }
    // wave sum
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) cnt += (u64)__shfl_xor((long long)cnt, s, BG_WAVE);
    if (lane_id() == 0) wave_counts[c] = cnt;
  }
}

__global__ void k_mask_scatter(const u64* words, int64_t nwords, int64_t n,
                               const i64* chunk_offsets, int64_t nchunks,
                               uint32_t* out) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t c = wave_global; c < nchunks; c += nwaves) {
    const int64_t w0 = c * MC_WORDS_PER_WAVE;
    const int64_t w1 = min(w0 + (int64_t)MC_WORDS_PER_WAVE, nwords);
    i64 base = chunk_offsets[c];
    for (int64_t w = w0; w < w1; ++w) {  // in order => stability
      u64 m = words[w];
      if (w == nwords - 1 && (n & 63)) m &= (1ull << (n & 63)) - 1;
      const int l = lane_id();
      if ((m >> l) & 1) {
        int pos = __popcll(m & ((1ull << l) - 1));
        out[base + pos] = (uint32_t)(w * BG_WAVE + l);
      }
      base += __popcll(m);
    }
  }
}

// d_indices == nullptr: count only (the scatter pass is skipped)
static int mask_to_indices(const uint8_t* d_mask, int64_t n,
                           uint32_t* d_indices, int64_t* out_count) {
  const int64_t nwords = (n + 63) / 64;
  const int64_t nchunks = (nwords + MC_WORDS_PER_WAVE - 1) / MC_WORDS_PER_WAVE;
  DevBuf<u64> d_counts;
  DevBuf<i64> d_offs;
  DevBuf<i64> d_total;
  HIP_TRY(d_counts.alloc(nchunks));
  HIP_TRY(d_offs.alloc(nchunks));
  HIP_TRY(d_total.alloc(1));
  int blocks = grid_for(nchunks, 1);
  hipLaunchKernelGGL(k_mask_count, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     reinterpret_cast<const u64*>(d_mask), nwords, n, d_counts,
                     nchunks);
  {
    int rc = scan_exclusive_i64(d_counts, nchunks, d_offs, d_total);
    if (rc != BG_OK) return rc;
  }
  if (d_indices)
    hipLaunchKernelGGL(k_mask_scatter, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                       reinterpret_cast<const u64*>(d_mask), nwords, n, d_offs,
                       nchunks, d_indices);
  i64 total = 0;
  HIP_TRY(hipMemcpy(&total, d_total, sizeof(i64), hipMemcpyDeviceToHost));
  *out_count = total;
  return BG_OK;
}

extern "C" int bg_mask_to_indices(const uint8_t* d_mask, int64_t n,
                                  uint32_t* d_indices, int64_t* out_count) {
  REQUIRE_INIT();
  return mask_to_indices(d_mask, n, d_indices, out_count);
}

// ---------------------------------------------------------------------------
// gather (take)
// ---------------------------------------------------------------------------
template <typename T>
__global__ void k_gather(const T* src, const uint32_t* idx, int64_t m, T* dst) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = src[idx[i]];
}

extern "C" int bg_gather(const void* d_src, int64_t elem_size,
                         const uint32_t* d_idx, int64_t m, void* d_dst) {
  REQUIRE_INIT();
  int blocks = grid_for(m);
  switch (elem_size) {
    case 1:
      hipLaunchKernelGGL(k_gather<uint8_t>, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                         (const uint8_t*)d_src, d_idx, m, (uint8_t*)d_dst);
      break;
    case 2:
      hipLaunchKernelGGL(k_gather<uint16_t>, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                         (const uint16_t*)d_src, d_idx, m, (uint16_t*)d_dst);
      break;
    case 4:
      hipLaunchKernelGGL(k_gather<uint32_t>, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                         (const uint32_t*)d_src, d_idx, m, (uint32_t*)d_dst);
      break;
    case 8:
      hipLaunchKernelGGL(k_gather<u64>, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                         (const u64*)d_src, d_idx, m, (u64*)d_dst);
      break;
    case 16:
      hipLaunchKernelGGL(k_gather<ulong2>, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                         (const ulong2*)d_src, d_idx, m, (ulong2*)d_dst);
      break;
    default:
      return set_err(BG_ERR_INVALID, "elem_size must be 1/2/4/8/16");
  }
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---------------------------------------------------------------------------
// create_hashes (bg_ahash.h restatement) + partition ids
// ---------------------------------------------------------------------------
struct KeyArgs {
  int nkeys;
  struct {
    const void* data;
    const uint8_t* valid;
    const int32_t* offsets;  // UTF8 only
    int dtype;
  } k[BG_MAX_KEYS];
};

__global__ void k_hash_columns(KeyArgs keys, int64_t n, u64* hashes) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    u64 h = 0;
    for (int c = 0; c < keys.nkeys; ++c) {
      if (!bit_valid(keys.k[c].valid, i)) continue;  // null: leave running hash
      u64 hc;
      switch (keys.k[c].dtype) {
        case BG_DT_INT64:
          hc = bg_hash_u64((u64)__builtin_nontemporal_load(
              reinterpret_cast<const int64_t*>(keys.k[c].data) + i));
          break;
        case BG_DT_INT32:
        case BG_DT_DATE32:
          hc = bg_hash_u32((uint32_t)__builtin_nontemporal_load(
              reinterpret_cast<const int32_t*>(keys.k[c].data) + i));
          break;
        case BG_DT_DECIMAL128: {
          typedef unsigned long long ull2_ev
              __attribute__((ext_vector_type(2)));
          const ull2_ev v = __builtin_nontemporal_load(
              reinterpret_cast<const ull2_ev*>(keys.k[c].data) + i);
          hc = bg_hash_u128(v[0], v[1]);
          break;
        }
        case BG_DT_DICT8:
          // dictionary codes hash as their u8 value zero-extended (the host
          // maps codes back to dictionary values before hashing when exact
          // Utf8 hash parity is required; DICT8 here is for synthetic keys)
          hc = bg_hash_u64((u64) reinterpret_cast<const uint8_t*>(keys.k[c].data)[i]);
          break;
        case BG_DT_UTF8: {
          const int32_t lo = keys.k[c].offsets[i];
          const int32_t hi_off = keys.k[c].offsets[i + 1];
          hc = bg_hash_str(
              reinterpret_cast<const uint8_t*>(keys.k[c].data) + lo,
              (uint64_t)(hi_off - lo));
          break;
        }
        default:
          hc = 0;
      }
      h = (c == 0) ? hc : bg_combine_hashes(hc, h);
    }
    hashes[i] = h;
  }
}

extern "C" int bg_hash_columns(const bg_column* key_cols, int32_t nkeys,
                               int64_t n, uint64_t* d_hashes) {
  REQUIRE_INIT();
  if (nkeys <= 0 || nkeys > BG_MAX_KEYS)
    return set_err(BG_ERR_INVALID, "nkeys out of range [1,4]");
  KeyArgs a{};
  a.nkeys = nkeys;
  for (int i = 0; i < nkeys; ++i) {
    a.k[i].data = key_cols[i].d_data;
    a.k[i].valid = key_cols[i].d_validity;
    a.k[i].offsets = key_cols[i].d_offsets;
    a.k[i].dtype = key_cols[i].dtype;
  }
  int blocks = grid_for(n);
  hipLaunchKernelGGL(k_hash_columns, dim3(blocks), dim3(BG_BLOCK), 0, 0, a, n,
                     reinterpret_cast<u64*>(d_hashes));
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

__global__ void k_partition_ids(const u64* hashes, int64_t n, uint32_t k,
                                uint32_t* pids) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    pids[i] = (uint32_t)(hashes[i] % (u64)k);
}

extern "C" int bg_partition_ids(const uint64_t* d_hashes, int64_t n, uint32_t k,
                                uint32_t* d_pids) {
  REQUIRE_INIT();
  if (k == 0) return set_err(BG_ERR_INVALID, "k == 0");
  int blocks = grid_for(n);
  hipLaunchKernelGGL(k_partition_ids, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     reinterpret_cast<const u64*>(d_hashes), n, k, d_pids);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---------------------------------------------------------------------------
// stable multi-split (compute_partition_indices device equivalent)
// layout: hist[p * nchunks + c] -> p-major so the exclusive scan directly
// yields each (partition, chunk) start and offsets[p] = scan[p * nchunks].
// ---------------------------------------------------------------------------
#define PS_ROWS_PER_WAVE 16384

__global__ void k_part_hist(const uint32_t* pids, int64_t n, uint32_t k,
                            u64* hist, int64_t nchunks) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  // per-wave counters: waves_per_block * k u32
  uint32_t* cnt = reinterpret_cast<uint32_t*>(smem_raw);
  const int wave_in_block = threadIdx.x / BG_WAVE;
  uint32_t* my = cnt + (size_t)wave_in_block * k;
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t c = wave_global; c < nchunks; c += nwaves) {
    for (uint32_t p = lane_id(); p < k; p += BG_WAVE) my[p] = 0;
    __builtin_amdgcn_wave_barrier();
    const int64_t r0 = c * PS_ROWS_PER_WAVE;
    const int64_t r1 = min(r0 + (int64_t)PS_ROWS_PER_WAVE, n);
    for (int64_t r = r0 + lane_id(); r < r1; r += BG_WAVE)
      atomicAdd(&my[pids[r]], 1u);
    __builtin_amdgcn_wave_barrier();
    for (uint32_t p = lane_id(); p < k; p += BG_WAVE)
      hist[(int64_t)p * nchunks + c] = my[p];
  }
}

__global__ void k_part_scatter(const uint32_t* pids, int64_t n, uint32_t k,
                               const i64* start, int64_t nchunks,
                               uint32_t* out, uint32_t* rank /*optional*/) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  i64* cur = reinterpret_cast<i64*>(smem_raw);  // waves_per_block * k
  const int wave_in_block = threadIdx.x / BG_WAVE;
  i64* my = cur + (size_t)wave_in_block * k;
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t c = wave_global; c < nchunks; c += nwaves) {
    for (uint32_t p = lane_id(); p < k; p += BG_WAVE)
      my[p] = start[(int64_t)p * nchunks + c];
    __builtin_amdgcn_wave_barrier();
    // register cursors for the k<=64 fast path (lane p owns partition p)
    int cur_lo = 0, cur_hi = 0;
    if (k <= BG_WAVE) {
      const i64 seed = (lane_id() < (int)k)
                           ? start[(int64_t)lane_id() * nchunks + c]
                           : 0;
      cur_lo = (int)(uint32_t)((u64)seed & 0xffffffff);
      cur_hi = (int)(uint32_t)((u64)seed >> 32);
    }
    const int64_t r0 = c * PS_ROWS_PER_WAVE;
    const int64_t r1 = min(r0 + (int64_t)PS_ROWS_PER_WAVE, n);
    for (int64_t rb = r0; rb < r1; rb += BG_WAVE) {
      const int64_t r = rb + lane_id();
      const bool active = r < r1;
      const uint32_t pid = active ? pids[r] : 0xffffffffu;
      i64 my_pos = -1;
      if (k <= BG_WAVE) {
        // dense partition loop with REGISTER cursors: lane p's element of
        // `cur_lane` holds partition p's cursor; readlane/writelane avoid
        // the ~50-cycle LDS round trip per partition iteration that
        // serialises the whole wave (cursors were seeded from LDS `my`
        // before the row loop)
        for (uint32_t p = 0; p < k; ++p) {
          const u64 m = __ballot(active && pid == p);
          if (!m) continue;
          const i64 base =
              ((i64)(uint32_t)__builtin_amdgcn_readlane(cur_hi, p) << 32) |
              (i64)(uint32_t)__builtin_amdgcn_readlane(cur_lo, p);
          if (active && pid == p)
            my_pos = base + __popcll(m & ((1ull << lane_id()) - 1));
          const i64 nxt = base + __popcll(m);
          // per-lane select: lane p adopts the new cursor (nxt is wave-
          // uniform; one v_cndmask per word, no LDS round trip)
          const bool mine = (uint32_t)lane_id() == p;
          cur_lo = mine ? (int)(uint32_t)((u64)nxt & 0xffffffff) : cur_lo;
          cur_hi = mine ? (int)(uint32_t)((u64)nxt >> 32) : cur_hi;
        }
      } else {
        // ballot-bit multi-split (ceil(log2 k) ballots give each lane the
        // mask of lanes sharing its partition) — replaces the serialized
        // per-distinct-partition leader loop
        const u64 act = __ballot(active);
        u64 same = act;
        const int nbits = 32 - __builtin_clz(k - 1);
        for (int b = 0; b < nbits; ++b) {
          const u64 bb = __ballot(((pid >> b) & 1u) != 0u);
          same &= ((pid >> b) & 1u) ? bb : ~bb;
        }
        if (active) {
          const u64 lower = same & ((1ull << lane_id()) - 1);
          const i64 base = my[pid];
          my_pos = base + __popcll(lower);
          __builtin_amdgcn_wave_barrier();
          if (lower == 0) my[pid] = base + __popcll(same);
        }
        __builtin_amdgcn_wave_barrier();
      }
      if (active) {
        out[my_pos] = (uint32_t)r;
        if (rank) rank[r] = (uint32_t)my_pos;  // coalesced inverse perm
      }
    }
  }
}

__global__ void k_extract_offsets(const i64* start, int64_t nchunks, uint32_t k,
                                  int64_t n, int64_t* offsets) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p <= k;
       p += gridDim.x * blockDim.x)
    offsets[p] = (p == k) ? n : start[(int64_t)p * nchunks];
}

extern "C" int bg_partition_indices_ex(const uint32_t* d_pids, int64_t n,
                                       uint32_t k, uint32_t* d_indices,
                                       int64_t* d_offsets, uint32_t* d_rank) {
  REQUIRE_INIT();
  if (k == 0 || k > 4096) return set_err(BG_ERR_INVALID, "k out of range [1,4096]");
  const int64_t nchunks = (n + PS_ROWS_PER_WAVE - 1) / PS_ROWS_PER_WAVE;
  const int waves_per_block = BG_BLOCK / BG_WAVE;
  const size_t lds_hist = (size_t)waves_per_block * k * sizeof(uint32_t);
  const size_t lds_scat = (size_t)waves_per_block * k * sizeof(i64);
  DevBuf<u64> d_hist;
  DevBuf<i64> d_start;
  const int64_t hist_len = (int64_t)k * (nchunks ? nchunks : 1);
  HIP_TRY(d_hist.alloc(hist_len));
  HIP_TRY(d_start.alloc(hist_len));
  int blocks = grid_for(nchunks, 1);
  hipLaunchKernelGGL(k_part_hist, dim3(blocks), dim3(BG_BLOCK), lds_hist, 0,
                     d_pids, n, k, d_hist, nchunks);
  {
    int rc = scan_exclusive_i64(d_hist, hist_len, d_start, nullptr);
    if (rc != BG_OK) return rc;
  }
  hipLaunchKernelGGL(k_extract_offsets, dim3(1), dim3(BG_BLOCK), 0, 0, d_start,
                     nchunks, k, n, d_offsets);
  hipLaunchKernelGGL(k_part_scatter, dim3(blocks), dim3(BG_BLOCK), lds_scat, 0,
                     d_pids, n, k, d_start, nchunks, d_indices, d_rank);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return BG_OK;
}

extern "C" int bg_partition_indices(const uint32_t* d_pids, int64_t n,
                                    uint32_t k, uint32_t* d_indices,
                                    int64_t* d_offsets) {
  return bg_partition_indices_ex(d_pids, n, k, d_indices, d_offsets, nullptr);
}

// scatter-materialise: dst[rank[i]] = src[i] (sequential reads, partition-
// major writes into <= k streams — avoids the gather's k-fold read
// amplification on the permuted side)
template <typename T>
__global__ void k_scatter_rows(const T* src, const uint32_t* rank, int64_t n,
                               T* dst) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    // sequential inputs are read once: non-temporal; the scattered writes
    // stay cached so partial lines combine in L2
    const uint32_t r = __builtin_nontemporal_load(&rank[i]);
    dst[r] = src[i];
  }
}

extern "C" int bg_scatter_rows(const void* d_src, int64_t elem_size,
                               const uint32_t* d_rank, int64_t n,
                               void* d_dst) {
  REQUIRE_INIT();
  int blocks = grid_for(n);
  switch (elem_size) {
    case 1:
      hipLaunchKernelGGL(k_scatter_rows<uint8_t>, dim3(blocks), dim3(BG_BLOCK),
                         0, 0, (const uint8_t*)d_src, d_rank, n, (uint8_t*)d_dst);
      break;
    case 4:
      hipLaunchKernelGGL(k_scatter_rows<uint32_t>, dim3(blocks), dim3(BG_BLOCK),
                         0, 0, (const uint32_t*)d_src, d_rank, n, (uint32_t*)d_dst);
      break;
    case 8:
      hipLaunchKernelGGL(k_scatter_rows<u64>, dim3(blocks), dim3(BG_BLOCK),
                         0, 0, (const u64*)d_src, d_rank, n, (u64*)d_dst);
      break;
    case 16:
      hipLaunchKernelGGL(k_scatter_rows<ulong2>, dim3(blocks), dim3(BG_BLOCK),
                         0, 0, (const ulong2*)d_src, d_rank, n, (ulong2*)d_dst);
      break;
    default:
      return set_err(BG_ERR_INVALID, "elem_size must be 1/4/8/16");
  }
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

static int64_t dtype_size(int dtype) {
  switch (dtype) {
    case BG_DT_INT32:
    case BG_DT_DATE32: return 4;
    case BG_DT_INT64: return 8;
    case BG_DT_DECIMAL128: return 16;
    case BG_DT_DICT8: return 1;
    default: return 0;
  }
}

extern "C" int bg_hash_repartition(const bg_column* key_cols, int32_t nkeys,
                                   const bg_column* payload_cols, int32_t ncols,
                                   int64_t n, uint32_t k, uint32_t* d_indices,
                                   int64_t* d_offsets, void** d_out) {
  REQUIRE_INIT();
  if (ncols > BG_MAX_PAYLOAD) return set_err(BG_ERR_INVALID, "too many payload cols");
  DevBuf<uint64_t> d_hashes;
  DevBuf<uint32_t> d_pids;
  DevBuf<uint32_t> d_rank;
  HIP_TRY(d_hashes.alloc(n));
  HIP_TRY(d_pids.alloc(n));
  HIP_TRY(d_rank.alloc(n));
  int rc = bg_hash_columns(key_cols, nkeys, n, d_hashes);
  if (rc == BG_OK) rc = bg_partition_ids(d_hashes, n, k, d_pids);
  if (rc == BG_OK)
    rc = bg_partition_indices_ex(d_pids, n, k, d_indices, d_offsets, d_rank);
  for (int c = 0; c < ncols && rc == BG_OK; ++c) {
    int64_t esz = dtype_size(payload_cols[c].dtype);
    if (esz == 0) return set_err(BG_ERR_UNSUPPORTED, "payload dtype");
    // sequential-read scatter through the inverse permutation
    rc = bg_scatter_rows(payload_cols[c].d_data, esz, d_rank, n, d_out[c]);
  }
  return rc;
}

// ---------------------------------------------------------------------------
// q6: fused scan + filter + SUM(l_extendedprice * l_discount)
//
// Staged short-circuit scan.  The predicate is a conjunction of pure
// comparisons, so a row that fails the date window can never need its
// discount, and one that fails date or discount can never need its
// quantity.  Columns are loaded in the order shipdate -> discount ->
// quantity -> extendedprice, each only by lanes whose row passed every
// earlier test; the memory pipeline fetches a 128-B line only if a live
// lane addresses it, so HBM traffic is 4 B/row of dates plus the lines of
// each later column that hold a survivor (TPC-H q6: 14.4 % / 3.9 % / 1.8 %
// of rows survive the three tests) instead of 36 B/row + price lines.
//
// Done row-at-a-time that is four dependent HBM round trips, so each thread
// owns BG_Q6_U rows of a BG_BLOCK*BG_Q6_U-row tile (row = tile_base +
// u*BG_BLOCK + threadIdx.x: every wave instruction stays contiguous, 256 B
// of dates / 1 KB of decimals) and a stage issues all of its loads before
// any of them is consumed.  Comparisons stay on the full 128-bit value.
// Column bases are only assumed element-aligned (4 B / 16 B).
// ---------------------------------------------------------------------------
#ifndef BG_Q6_U
#define BG_Q6_U 8
#endif

// One Decimal128 as a clang vector: stays one 4-VGPR tuple from the load to
// its use (HIP_vector_type isn't a clang vector and would be split).
typedef unsigned long long q6_dec __attribute__((ext_vector_type(2)));

template <bool NT>
__device__ __forceinline__ q6_dec q6_load_dec(const ulong2* p) {
  // NT: every byte is read at most once per pass — non-temporal loads skip
  // L2 retention.
  const q6_dec* q = reinterpret_cast<const q6_dec*>(p);
  return NT ? __builtin_nontemporal_load(q) : *q;
}

// Stage boundary: every value of the finished stage is pinned in its
// register here, so the compiler waits for the whole stage once and cannot
// sink one row's test between the next stage's loads — where, loads
// returning in order, the wait would also cover the loads just issued.
__device__ __forceinline__ void q6_stage_end(int32_t (&d)[BG_Q6_U]) {
#pragma unroll
  for (int u = 0; u < BG_Q6_U; ++u) asm volatile("" : "+v"(d[u]) : : "memory");
}
__device__ __forceinline__ void q6_stage_end(q6_dec (&v)[BG_Q6_U]) {
#pragma unroll
  for (int u = 0; u < BG_Q6_U; ++u) asm volatile("" : "+v"(v[u]) : : "memory");
}

// Stage 1 of one tile: U date loads per thread, nothing consumed.  The loads
// are unconditional — a row past the end reads row n-1 instead and is
// discarded by the caller's `i < n` test — so their number is the same on
// every path and the compiler's wait counts stay exact.  Needs n >= 1.
template <bool NT>
__device__ __forceinline__ void q6_load_dates(const int32_t* shipdate,
                                              int64_t row0, int64_t n,
                                              int32_t (&d)[BG_Q6_U]) {
#pragma unroll
  for (int u = 0; u < BG_Q6_U; ++u) {
    int64_t i = row0 + (int64_t)u * BG_BLOCK;
    if (i >= n) i = n - 1;
    d[u] = NT ? __builtin_nontemporal_load(&shipdate[i]) : shipdate[i];
  }
}

template <bool NT>
__global__ __launch_bounds__(BG_BLOCK) void k_q6_agg(
    const int32_t* shipdate, const ulong2* discount, const ulong2* quantity,
    const ulong2* extendedprice, int64_t n, int32_t date_lo, int32_t date_hi,
    i64 disc_lo, i64 disc_hi, i64 qty_lt, u64* out_lo, u64* out_hi,
    u64* out_count) {
  constexpr int U = BG_Q6_U;
  constexpr int64_t T = (int64_t)BG_BLOCK * U;
  const int64_t ntiles = (n + T - 1) / T;
  i128 acc = 0;
  u64 cnt = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * T + threadIdx.x;
    // stage 1: dates
    int32_t d[U];
    q6_load_dates<NT>(shipdate, row0, n, d);
    q6_stage_end(d);
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      live[u] = (row0 + (int64_t)u * BG_BLOCK < n) & (d[u] >= date_lo) &
                (d[u] < date_hi);
    // stage 2: discount, only where the date passed
    q6_dec v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = q6_dec{0, 0};
      if (live[u])
        v[u] = q6_load_dec<NT>(discount + row0 + (int64_t)u * BG_BLOCK);
    }
    q6_stage_end(v);
    // a discount inside [disc_lo, disc_hi] fits i64: keep the low limb only
    i64 disc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const i128 x = make_i128(v[u][0], (i64)v[u][1]);
      live[u] = live[u] & (x >= disc_lo) & (x <= disc_hi);
      disc[u] = (i64)v[u][0];
    }
    // stage 3: quantity, only where date and discount passed
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = q6_dec{0, 0};
      if (live[u])
        v[u] = q6_load_dec<NT>(quantity + row0 + (int64_t)u * BG_BLOCK);
    }
    q6_stage_end(v);
#pragma unroll
    for (int u = 0; u < U; ++u)
      live[u] = live[u] & (make_i128(v[u][0], (i64)v[u][1]) < qty_lt);
    // stage 4: price, only for selected rows
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = q6_dec{0, 0};
      if (live[u])
        v[u] = q6_load_dec<NT>(extendedprice + row0 + (int64_t)u * BG_BLOCK);
    }
    q6_stage_end(v);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (live[u]) {
        acc += make_i128(v[u][0], (i64)v[u][1]) * (i128)disc[u];
        cnt++;
      }
    }
  }
  // wave -> block -> global
  acc = wave_reduce_i128(acc);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) cnt += (u64)__shfl_xor((long long)cnt, s, BG_WAVE);
  __shared__ u64 slo[BG_BLOCK / BG_WAVE], shi[BG_BLOCK / BG_WAVE],
      scnt[BG_BLOCK / BG_WAVE];
  const int w = threadIdx.x / BG_WAVE;
  if (lane_id() == 0) {
    slo[w] = (u64)(u128)acc;
    shi[w] = (u64)((u128)acc >> 64);
    scnt[w] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    i128 bacc = 0;
    u64 bcnt = 0;
    for (int i = 0; i < BG_BLOCK / BG_WAVE; ++i) {
      bacc += make_i128(slo[i], (i64)shi[i]);
      bcnt += scnt[i];
    }
    atomic_add_i128(out_lo, out_hi, bacc);
    atomicAdd(out_count, bcnt);
  }
}

// Per-thread fixed state of bg_q6_agg: at ~2 ms per call, creating and
// destroying two events, a blocking memset and a pageable copy per call are
// no longer noise.  Events and the pinned result words are made once per
// (thread, device) and reused.
struct Q6HostState {
  int device = -1;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  u64* h_res = nullptr;  // pinned [lo, hi, count]
};
static thread_local Q6HostState g_q6;

static int q6_host_state(Q6HostState** out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (g_q6.device != dev) {
    if (g_q6.device >= 0) {  // the thread moved to another device
      (void)hipEventDestroy(g_q6.ev0);
      (void)hipEventDestroy(g_q6.ev1);
      (void)hipHostFree(g_q6.h_res);
      g_q6 = Q6HostState();
    }
    Q6HostState st;
    HIP_TRY(hipEventCreate(&st.ev0));
    HIP_TRY(hipEventCreate(&st.ev1));
    HIP_TRY(hipHostMalloc((void**)&st.h_res, 3 * sizeof(u64)));
    st.device = dev;
    g_q6 = st;
  }
  *out = &g_q6;
  return BG_OK;
}

extern "C" int bg_q6_agg(const bg_column* shipdate, const bg_column* discount,
                         const bg_column* quantity,
                         const bg_column* extendedprice, int32_t date_lo,
                         int32_t date_hi, int64_t disc_lo, int64_t disc_hi,
                         int64_t qty_lt, uint64_t* out_sum_lo,
                         int64_t* out_sum_hi, int64_t* out_count) {
  REQUIRE_INIT();
  if (shipdate->dtype != BG_DT_DATE32 && shipdate->dtype != BG_DT_INT32)
    return set_err(BG_ERR_INVALID, "shipdate must be DATE32");
  const int64_t n = shipdate->len;
  Q6HostState* st;
  if (int rc = q6_host_state(&st)) return rc;
  u64* d_acc;  // [lo, hi, count]
  HIP_TRY(pool_malloc((void**)&d_acc, 3 * sizeof(u64)));
  HIP_TRY(hipMemsetAsync(d_acc, 0, 3 * sizeof(u64), 0));
  // one block per tile, grid-stride beyond the cap
  const int64_t tile = (int64_t)BG_BLOCK * BG_Q6_U;
  int blocks = grid_for(n, tile);
  HIP_TRY(hipEventRecord(st->ev0, 0));
  // non-temporal loads by default: the fused scan reads every byte at most
  // once, and NT streams measured +11% over cached loads (6.7 vs 6.05 TB/s)
  static const bool use_nt = [] {
    const char* e = getenv("BG_Q6_NT");
    return !(e && e[0] == '0');
  }();
  if (use_nt)
    hipLaunchKernelGGL(k_q6_agg<true>, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                       (const int32_t*)shipdate->d_data,
                       (const ulong2*)discount->d_data,
                       (const ulong2*)quantity->d_data,
                       (const ulong2*)extendedprice->d_data, n, date_lo,
                       date_hi, disc_lo, disc_hi, qty_lt, d_acc, d_acc + 1,
                       d_acc + 2);
  else
    hipLaunchKernelGGL(k_q6_agg<false>, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                       (const int32_t*)shipdate->d_data,
                       (const ulong2*)discount->d_data,
                       (const ulong2*)quantity->d_data,
                       (const ulong2*)extendedprice->d_data, n, date_lo,
                       date_hi, disc_lo, disc_hi, qty_lt, d_acc, d_acc + 1,
                       d_acc + 2);
  HIP_TRY(hipGetLastError());
  // ev0/ev1 bracket the kernel alone; the readback rides behind ev1
  HIP_TRY(hipEventRecord(st->ev1, 0));
  HIP_TRY(hipMemcpyAsync(st->h_res, d_acc, 3 * sizeof(u64),
                         hipMemcpyDeviceToHost, 0));
  HIP_TRY(hipStreamSynchronize(0));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, st->ev0, st->ev1));
  g_last_kernel_ms = (double)ms;
  HIP_TRY(pool_release(d_acc));
  *out_sum_lo = st->h_res[0];
  *out_sum_hi = (int64_t)st->h_res[1];
  *out_count = (int64_t)st->h_res[2];
  return BG_OK;
}

// ---------------------------------------------------------------------------
// q1: fused filter + grouped partial aggregate.
// Wave-clustered: per 64 rows, loop over the distinct groups present
// (ballot leader loop — 4 in TPC-H q1), full-wave register reductions, one
// LDS atomic set per (group, iteration); block LDS table flushed once.
// 70 B/row algorithmic (2 x u8 + 4 x Decimal128 + Date32).
// ---------------------------------------------------------------------------
#define Q1_GROUPS 256
#define Q1_ACCS 5  // qty, price, disc_price, charge, disc

__global__ void k_q1_agg(const uint8_t* rf, const uint8_t* ls,
                         const ulong2* quantity, const ulong2* extendedprice,
                         const ulong2* discount, const ulong2* tax,
                         const int32_t* shipdate, int64_t n, int32_t date_le,
                         u64* g_sums /*Q1_GROUPS*Q1_ACCS*2*/,
                         u64* g_counts /*Q1_GROUPS*/) {
  // Per-block LDS accumulators, one u64 per (group, acc): Decimal128(15,2)
  // row values fit i64 (|v| < 10^15), and per-block partial sums stay
  // < 2^63 for any block processing <= ~10^6 rows (grid sizing guarantees
  // this), so block-local accumulation needs no i128 carries — one
  // no-return ds_add per acc per row.  The i128 exactness is restored at
  // the block flush (sign-extended i64 partial -> global carry atomics).
  __shared__ u64 s_sums[Q1_GROUPS * Q1_ACCS];
  __shared__ u64 s_counts[Q1_GROUPS];
  for (int i = threadIdx.x; i < Q1_GROUPS * Q1_ACCS; i += blockDim.x)
    s_sums[i] = 0;
  for (int i = threadIdx.x; i < Q1_GROUPS; i += blockDim.x) s_counts[i] = 0;
  __syncthreads();

  typedef unsigned long long ull2_ev __attribute__((ext_vector_type(2)));
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    // non-temporal: every stream byte is read exactly once per pass
    if (__builtin_nontemporal_load(&shipdate[i]) > date_le) continue;
    const uint32_t g =
        ((uint32_t)__builtin_nontemporal_load(&rf[i]) << 4) |
        (uint32_t)__builtin_nontemporal_load(&ls[i]);
    const i64 qty = (i64)__builtin_nontemporal_load(
        reinterpret_cast<const ull2_ev*>(quantity) + i)[0];
    const i64 price = (i64)__builtin_nontemporal_load(
        reinterpret_cast<const ull2_ev*>(extendedprice) + i)[0];
    const i64 disc = (i64)__builtin_nontemporal_load(
        reinterpret_cast<const ull2_ev*>(discount) + i)[0];
    const i64 tx = (i64)__builtin_nontemporal_load(
        reinterpret_cast<const ull2_ev*>(tax) + i)[0];
    const i64 disc_price = price * (100 - disc);
    u64* base = &s_sums[g * Q1_ACCS];
    atomicAdd(&base[0], (u64)qty);
    atomicAdd(&base[1], (u64)price);
    atomicAdd(&base[2], (u64)disc_price);
    atomicAdd(&base[3], (u64)(disc_price * (100 + tx)));
    atomicAdd(&base[4], (u64)disc);
    atomicAdd(&s_counts[g], 1ull);
  }
  __syncthreads();
  for (int gidx = threadIdx.x; gidx < Q1_GROUPS; gidx += blockDim.x) {
    if (s_counts[gidx]) atomicAdd(&g_counts[gidx], s_counts[gidx]);
    for (int a = 0; a < Q1_ACCS; ++a) {
      const i64 v = (i64)s_sums[gidx * Q1_ACCS + a];
      if (v)
        atomic_add_i128(&g_sums[(gidx * Q1_ACCS + a) * 2],
                        &g_sums[(gidx * Q1_ACCS + a) * 2 + 1], (i128)v);
    }
  }
}

extern "C" int bg_q1_agg(const bg_column* rf, const bg_column* ls,
                         const bg_column* quantity,
                         const bg_column* extendedprice,
                         const bg_column* discount, const bg_column* tax,
                         const bg_column* shipdate, int32_t date_le,
                         int64_t* h_counts, uint8_t* h_sums) {
  REQUIRE_INIT();
  const int64_t n = shipdate->len;
  DevBuf<u64> d_sums, d_counts;
  HIP_TRY(d_sums.alloc(Q1_GROUPS * Q1_ACCS * 2));
  HIP_TRY(d_counts.alloc(Q1_GROUPS));
  HIP_TRY(hipMemset(d_sums, 0, Q1_GROUPS * Q1_ACCS * 2 * sizeof(u64)));
  HIP_TRY(hipMemset(d_counts, 0, Q1_GROUPS * sizeof(u64)));
  int blocks = grid_for(n);
  EventPair ev;
  HIP_TRY(ev.create());
  HIP_TRY(hipEventRecord(ev.ev0, 0));
  hipLaunchKernelGGL(k_q1_agg, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (const uint8_t*)rf->d_data, (const uint8_t*)ls->d_data,
                     (const ulong2*)quantity->d_data,
                     (const ulong2*)extendedprice->d_data,
                     (const ulong2*)discount->d_data,
                     (const ulong2*)tax->d_data,
                     (const int32_t*)shipdate->d_data, n, date_le, d_sums,
                     d_counts);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ev.ev1, 0));
  HIP_TRY(hipEventSynchronize(ev.ev1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.ev0, ev.ev1));
  g_last_kernel_ms = (double)ms;
  u64 sums[Q1_GROUPS * Q1_ACCS * 2];
  u64 counts[Q1_GROUPS];
  HIP_TRY(hipMemcpy(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost));
  for (int gidx = 0; gidx < Q1_GROUPS; ++gidx) {
    h_counts[gidx] = (int64_t)counts[gidx];
    for (int a = 0; a < Q1_ACCS; ++a) {
      memcpy(h_sums + (gidx * Q1_ACCS + a) * 16, &sums[(gidx * Q1_ACCS + a) * 2], 8);
      memcpy(h_sums + (gidx * Q1_ACCS + a) * 16 + 8,
             &sums[(gidx * Q1_ACCS + a) * 2 + 1], 8);
    }
  }
  return BG_OK;
}

// ---------------------------------------------------------------------------
// HashJoinExec build/probe (DataFusion 55 HashJoinExec
// partitioned-mode semantics for INNER equi-joins on integer keys).
// Chained hash table: head[nb] + next[n_build]; insertion via atomicExch is
// order-free (chain order is not part of the contract — SQL pins the result
// MULTISET; parity tests compare sorted pairs).  Probe is two-phase
// (count -> exclusive scan -> fill) so the output is probe-major with exact
// offsets and no atomic append nondeterminism in sizes.
// ---------------------------------------------------------------------------
struct BgJoinTable {
  ulong2* nodes;  // packed chain node: {key, next} — ONE line per hop
  int* head;      // bucket heads (-1 empty)
  int64_t n_build;
  u64 mask;       // nb - 1
  i64* probe_offsets = nullptr;  // per-probe-row output offsets (count phase)
  int64_t probe_n = 0;
};

__global__ void k_join_build(const int64_t* keys, const uint8_t* valid,
                             int64_t n, int* head, ulong2* nodes, u64 mask) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    // inner-join null semantics (null_equals_null=false in the reference's
    // HashJoinExec): a NULL build key matches nothing — leave it unlinked
    if (!bit_valid(valid, i)) continue;
    const u64 k = (u64)keys[i];
    const u64 b = bg_hash_u64(k) & mask;
    const int prev = atomicExch(&head[b], (int)i);
    ulong2 node;
    node.x = k;
    node.y = (u64)(int64_t)prev;  // sign-extended: -1 terminates
    nodes[i] = node;
  }
}

// 4-way ILP batching: each thread interleaves four independent chain
// walks so the ~900-cycle random node loads overlap (memory-level
// parallelism) instead of serialising per probe.
#define JOIN_ILP 4
__global__ void k_join_count(const int64_t* probe_keys,
                             const uint8_t* probe_valid, int64_t n_probe,
                             const int* head, const ulong2* nodes, u64 mask,
                             uint32_t* counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t base = tid; base < n_probe; base += stride * JOIN_ILP) {
    int64_t idx[JOIN_ILP];
    u64 key[JOIN_ILP];
    int64_t cur[JOIN_ILP];
    u64 cnt[JOIN_ILP];
#pragma unroll
    for (int j = 0; j < JOIN_ILP; ++j) {
      idx[j] = base + (int64_t)j * stride;
      const bool act = idx[j] < n_probe && bit_valid(probe_valid, idx[j]);
      key[j] = act ? (u64)probe_keys[idx[j]] : 0;
      cur[j] = act ? (int64_t)head[bg_hash_u64(key[j]) & mask] : -1;
      cnt[j] = 0;
    }
    bool any = true;
    while (any) {
      any = false;
#pragma unroll
      for (int j = 0; j < JOIN_ILP; ++j) {
        if (cur[j] >= 0) {
          const ulong2 node = nodes[cur[j]];
          if (node.x == key[j]) cnt[j]++;
          cur[j] = (int64_t)node.y;
          any = true;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < JOIN_ILP; ++j)
      if (idx[j] < n_probe) counts[idx[j]] = (uint32_t)cnt[j];
  }
}

__global__ void k_join_fill(const int64_t* probe_keys,
                             const uint8_t* probe_valid, int64_t n_probe,
                            const int* head, const ulong2* nodes, u64 mask,
                            const i64* offsets, uint32_t* out_probe,
                            uint32_t* out_build) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t base = tid; base < n_probe; base += stride * JOIN_ILP) {
    int64_t idx[JOIN_ILP];
    u64 key[JOIN_ILP];
    int64_t cur[JOIN_ILP];
    i64 w[JOIN_ILP];
#pragma unroll
    for (int j = 0; j < JOIN_ILP; ++j) {
      idx[j] = base + (int64_t)j * stride;
      const bool act = idx[j] < n_probe && bit_valid(probe_valid, idx[j]);
      key[j] = act ? (u64)probe_keys[idx[j]] : 0;
      cur[j] = act ? (int64_t)head[bg_hash_u64(key[j]) & mask] : -1;
      w[j] = act ? offsets[idx[j]] : 0;
    }
    bool any = true;
    while (any) {
      any = false;
#pragma unroll
      for (int j = 0; j < JOIN_ILP; ++j) {
        if (cur[j] >= 0) {
          const ulong2 node = nodes[cur[j]];
          if (node.x == key[j]) {
            out_probe[w[j]] = (uint32_t)idx[j];
            out_build[w[j]] = (uint32_t)cur[j];
            ++w[j];
          }
          cur[j] = (int64_t)node.y;
          any = true;
        }
      }
    }
  }
}

static u64 next_pow2_u64(u64 x) {
  u64 p = 1;
  while (p < x) p <<= 1;
  return p;
}

// The chained table of either join handle: mask for the smallest power of
// two of at least 2n buckets (8 at the least), head[] filled with -1, one
// node per build row.
static int join_alloc_table(int64_t n, u64* mask, DevBuf<int>* head,
                            DevBuf<ulong2>* nodes) {
  const u64 nb = next_pow2_u64((u64)(n > 4 ? n * 2 : 8));
  *mask = nb - 1;
  HIP_TRY(nodes->alloc(n));
  HIP_TRY(head->alloc((int64_t)nb));
  HIP_TRY(hipMemset(head->get(), 0xff, sizeof(int) * nb));  // -1
  return BG_OK;
}

// The count phase of either join handle once the call is checked:
// launch(counts) fills one u32 count per probe row, their exclusive scan
// becomes the offsets the handle keeps for the fill, the total goes to the
// caller.
template <typename Table, typename Launch>
static int join_count_phase(Table* t, int64_t n, int64_t* out_matches,
                            Launch&& launch) {
  // release the previous probe's offsets FIRST so the pool can recycle the
  // buffer for this call (allocating before releasing forces a fresh
  // multi-GB hipMalloc inside the hot path)
  if (t->probe_offsets) {
    (void)pool_release(t->probe_offsets);
    t->probe_offsets = nullptr;
  }
  DevBuf<uint32_t> d_counts;
  DevBuf<i64> d_offs;
  DevBuf<i64> d_total;
  HIP_TRY(d_counts.alloc(n));
  HIP_TRY(d_offs.alloc(n));
  HIP_TRY(d_total.alloc(1));
  launch(d_counts.get());
  HIP_TRY(hipGetLastError());
  // u32 counts: chains are < 2^31 long and per-row match counts fit —
  // halves the count write and the scan's level-0/3 read traffic
  int rc = scan_exclusive_u32(d_counts, n, d_offs, d_total);
  if (rc != BG_OK) return rc;
  i64 total = 0;
  HIP_TRY(hipMemcpy(&total, d_total, sizeof(i64), hipMemcpyDeviceToHost));
  // the handle owns the offsets until the next count or its free
  t->probe_offsets = d_offs.detach();
  t->probe_n = n;
  *out_matches = total;
  return BG_OK;
}

extern "C" int bg_hashjoin_build(const bg_column* build_keys, int64_t n,
                                 void** out_handle) {
  REQUIRE_INIT();
  if (build_keys->dtype != BG_DT_INT64)
    return set_err(BG_ERR_UNSUPPORTED, "join keys must be INT64 (round 1)");
  if (n > 0x7fffffffLL) return set_err(BG_ERR_INVALID, "build side > 2^31 rows");
  BgJoinTable t{};
  t.n_build = n;
  DevBuf<ulong2> nodes;
  DevBuf<int> head;
  int rc = join_alloc_table(n, &t.mask, &head, &nodes);
  if (rc != BG_OK) return rc;
  int blocks = grid_for(n);
  hipLaunchKernelGGL(k_join_build, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (const int64_t*)build_keys->d_data,
                     build_keys->d_validity, n, head.get(), nodes.get(),
                     t.mask);
  HIP_TRY(hipGetLastError());
  // the handle owns the table from here; bg_hashjoin_free releases it
  t.nodes = nodes.detach();
  t.head = head.detach();
  *out_handle = new BgJoinTable(t);
  return BG_OK;
}

extern "C" int bg_hashjoin_probe_count(void* handle,
                                       const bg_column* probe_keys, int64_t n,
                                       int64_t* out_matches) {
  REQUIRE_INIT();
  BgJoinTable* t = (BgJoinTable*)handle;
  if (probe_keys->dtype != BG_DT_INT64)
    return set_err(BG_ERR_UNSUPPORTED, "join keys must be INT64 (round 1)");
  return join_count_phase(t, n, out_matches, [&](uint32_t* d_counts) {
    hipLaunchKernelGGL(k_join_count, dim3(grid_for(n)), dim3(BG_BLOCK), 0, 0,
                       (const int64_t*)probe_keys->d_data,
                       probe_keys->d_validity, n, t->head, t->nodes, t->mask,
                       d_counts);
  });
}

extern "C" int bg_hashjoin_probe_fill(void* handle,
                                      const bg_column* probe_keys, int64_t n,
                                      uint32_t* d_out_probe,
                                      uint32_t* d_out_build) {
  REQUIRE_INIT();
  BgJoinTable* t = (BgJoinTable*)handle;
  if (!t->probe_offsets || t->probe_n != n)
    return set_err(BG_ERR_INVALID, "call bg_hashjoin_probe_count first");
  int blocks = grid_for(n);
  hipLaunchKernelGGL(k_join_fill, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (const int64_t*)probe_keys->d_data,
                     probe_keys->d_validity, n, t->head, t->nodes,
                     t->mask, t->probe_offsets, d_out_probe,
                     d_out_build);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

extern "C" int bg_hashjoin_free(void* handle) {
  REQUIRE_INIT();
  BgJoinTable* t = (BgJoinTable*)handle;
  if (!t) return BG_OK;
  (void)pool_release(t->nodes);
  (void)pool_release(t->head);
  if (t->probe_offsets) (void)pool_release(t->probe_offsets);
  delete t;
  return BG_OK;
}

// ---------------------------------------------------------------------------
// General hash group-by (AggregateExec Partial/Single for arbitrary group
// cardinality — SURVEY.md §8a row 2; q3-class: ~11.6M groups over 100M+
// rows).  Open-addressing table with linear probing; a slot stores the
// FIRST row index carrying its key (claimed with one atomicCAS) and the
// SLOT INDEX is the (sparse) group id — no group-counter handshake, no
// cross-workgroup spin on a second word (placement-independent by
// construction: claims and accumulations are device-scope atomics).
// Accumulators are slot-indexed; the host compacts occupied slots to dense
// groups with the existing mask->indices + gather machinery.
// ---------------------------------------------------------------------------
#define BG_MAX_AGGS 8
// MIN/MAX store an order-preserving u64 encoding with atomicMax so the
// zero-initialised slot is the identity (no per-slot init race):
//   MAX_I64: enc = v ^ (1<<63);          decode: enc ^ (1<<63)
//   MIN_I64: enc = ~(v ^ (1<<63));       decode: ~enc ^ (1<<63)
// (groups always hold >= 1 row, so enc 0 is never read back as a value)
// SUM over Float64: accumulation order is unordered (atomics), so low bits
// are nondeterministic — covered by the reference comparator's 1e-6
// relative float tolerance (benchmarks/src/lib.rs:35).
// MIN/MAX over Float64: totally-ordered u64 transform (negative values
// bit-inverted, positives sign-flipped — IEEE total order incl. infs),
// MIN stores the complement so atomicMax + zero identity works for both.

// MIN/MAX over Int32/Date32 (the I32 ops): the sign-extended value in the
// I64 encoding above — a 32-bit value fits it, so one atomicMax is enough.
// MIN/MAX over Decimal128/Utf8 (the ROW ops): no 128-bit atomic min/max
// exists and a string has no fixed width, so word 0 holds the WINNING
// INPUT ROW + 1 (0 = none yet, the claim word's encoding) and the value is
// gathered from that row afterwards.  A row replaces the holder with one
// CAS only where its value is STRICTLY better, so the word only improves,
// ties never swap and the loop ends; the input is read-only during the
// launch, so relaxed atomics suffice.  Which of several tied rows wins is
// not deterministic, the value gathered from it is.  Order: signed i128
// for Decimal128, bytewise unsigned lexicographic for Utf8 (Arrow's string
// order, as the reference's DataFusion Min/Max accumulators compare).

struct AggCol {
  const void* data;
  const uint8_t* valid;    // Arrow LSB validity or NULL (all valid)
  const int32_t* offsets;  // Utf8 only (the ROW ops compare through it)
  int op;
  int dtype;  // BG_DT_*: picks the ROW ops' comparison
};

struct AggArgs {
  int naggs;
  int vmode;  // 1: record carries a per-agg non-null count word (SQL needs
              // it to report SUM/MIN/MAX of an all-NULL group as NULL)
  AggCol a[BG_MAX_AGGS];
};

// three-way compare of rows r1, r2 of a Decimal128 or Utf8 column
__device__ __forceinline__ int agg_rows_cmp(const AggCol& c, int64_t r1,
                                            int64_t r2) {
  if (c.dtype == BG_DT_DECIMAL128) {
    const ulong2 a = reinterpret_cast<const ulong2*>(c.data)[r1];
    const ulong2 b = reinterpret_cast<const ulong2*>(c.data)[r2];
    // i128: high limb signed, low limb unsigned
    if (a.y != b.y) return (i64)a.y < (i64)b.y ? -1 : 1;
    if (a.x != b.x) return a.x < b.x ? -1 : 1;
    return 0;
  }
  const int32_t l1 = c.offsets[r1], n1 = c.offsets[r1 + 1] - l1;
  const int32_t l2 = c.offsets[r2], n2 = c.offsets[r2 + 1] - l2;
  const uint8_t* d = reinterpret_cast<const uint8_t*>(c.data);
  const int32_t m = n1 < n2 ? n1 : n2;
  for (int32_t j = 0; j < m; ++j) {
    const uint8_t x = d[l1 + j], y = d[l2 + j];
    if (x != y) return x < y ? -1 : 1;
  }
  // a proper prefix is smaller
  return n1 == n2 ? 0 : (n1 < n2 ? -1 : 1);
}

// MIN_ROW/MAX_ROW update of one accumulator word with candidate cand =
// row + 1.  SCOPE: agent for the global table, workgroup for an LDS table.
template <int SCOPE>
__device__ __forceinline__ void agg_row_update(u64* word, u64 cand,
                                               const AggCol& c) {
  const bool is_max = c.op == BG_AGG_OP_MAX_ROW;
  u64 cur = __hip_atomic_load(word, __ATOMIC_RELAXED, SCOPE);
  while (true) {
    if (cur != 0) {
      if (cur == cand) return;
      const int cmp = agg_rows_cmp(c, (int64_t)cand - 1, (int64_t)cur - 1);
      if (is_max ? cmp <= 0 : cmp >= 0) return;  // not strictly better
    }
    // on failure cur becomes the word's present value: compare again
    if (__hip_atomic_compare_exchange_strong(word, &cur, cand,
                                             __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, SCOPE))
      return;
  }
}

__device__ __forceinline__ bool keys_equal_rows(const KeyArgs& keys,
                                                int64_t r1, int64_t r2) {
  for (int c = 0; c < keys.nkeys; ++c) {
    // GROUP BY null semantics (group_values in the reference's DataFusion):
    // NULL groups with NULL; NULL never equals a value
    if (keys.k[c].valid) {
      const bool v1 = bit_valid(keys.k[c].valid, r1);
      const bool v2 = bit_valid(keys.k[c].valid, r2);
      if (v1 != v2) return false;
      if (!v1) continue;
    }
    switch (keys.k[c].dtype) {
      case BG_DT_INT64:
        if (reinterpret_cast<const int64_t*>(keys.k[c].data)[r1] !=
            reinterpret_cast<const int64_t*>(keys.k[c].data)[r2])
          return false;
        break;
      case BG_DT_INT32:
      case BG_DT_DATE32:
        if (reinterpret_cast<const int32_t*>(keys.k[c].data)[r1] !=
            reinterpret_cast<const int32_t*>(keys.k[c].data)[r2])
          return false;
        break;
      case BG_DT_DECIMAL128: {
        const ulong2 a = reinterpret_cast<const ulong2*>(keys.k[c].data)[r1];
        const ulong2 b = reinterpret_cast<const ulong2*>(keys.k[c].data)[r2];
        if (a.x != b.x || a.y != b.y) return false;
        break;
      }
      case BG_DT_DICT8:
        if (reinterpret_cast<const uint8_t*>(keys.k[c].data)[r1] !=
            reinterpret_cast<const uint8_t*>(keys.k[c].data)[r2])
          return false;
        break;
      case BG_DT_UTF8: {
        const int32_t* offs = keys.k[c].offsets;
        const int32_t l1 = offs[r1], h1 = offs[r1 + 1];
        const int32_t l2 = offs[r2], h2 = offs[r2 + 1];
        if (h1 - l1 != h2 - l2) return false;
        const uint8_t* d = reinterpret_cast<const uint8_t*>(keys.k[c].data);
        for (int32_t j = 0; j < h1 - l1; ++j)
          if (d[l1 + j] != d[l2 + j]) return false;
        break;
      }
      default:
        return false;
    }
  }
  return true;
}

__device__ __forceinline__ u64 hash_keys_row(const KeyArgs& keys, int64_t i) {
  u64 h = 0;
  for (int c = 0; c < keys.nkeys; ++c) {
    if (!bit_valid(keys.k[c].valid, i)) continue;  // null: leave running hash
    u64 hc;
    switch (keys.k[c].dtype) {
      case BG_DT_INT64:
        hc = bg_hash_u64((u64) reinterpret_cast<const int64_t*>(keys.k[c].data)[i]);
        break;
      case BG_DT_INT32:
      case BG_DT_DATE32:
        hc = bg_hash_u32((uint32_t) reinterpret_cast<const int32_t*>(keys.k[c].data)[i]);
        break;
      case BG_DT_DECIMAL128: {
        const ulong2 v = reinterpret_cast<const ulong2*>(keys.k[c].data)[i];
        hc = bg_hash_u128(v.x, v.y);
        break;
      }
      case BG_DT_DICT8:
        hc = bg_hash_u64((u64) reinterpret_cast<const uint8_t*>(keys.k[c].data)[i]);
        break;
      case BG_DT_UTF8: {
        // mirror k_hash_columns: without this, every Utf8 key row hashed
        // to one slot and the group-by degenerated to a single linear
        // chain
        const int32_t lo = keys.k[c].offsets[i];
        const int32_t hi_off = keys.k[c].offsets[i + 1];
        hc = bg_hash_str(reinterpret_cast<const uint8_t*>(keys.k[c].data) + lo,
                         (uint64_t)(hi_off - lo));
        break;
      }
      default:
        hc = 0;
    }
    h = (c == 0) ? hc : bg_combine_hashes(hc, h);
  }
  return h;
}

// slot_data: u64[cap * (2 + 2*naggs)] fully interleaved records
// [claim = first_row+1 (0 empty), count, acc0_lo, acc0_hi, ...] — the
// probe's claim word and the accumulators share ONE cache line per slot,
// so a row costs ~1 random line total (claim CAS/read + adds hit the same
// line); claims are device-scope u64 atomics (placement-independent)
__global__ void k_hashagg(KeyArgs keys, AggArgs aggs, const u64* mask_words,
                          int64_t n, u64 cap_mask, u64* slot_data,
                          int* err_flag) {
  const int wpa = 2 + aggs.vmode;  // words per agg in the slot record
  const int rec = 2 + wpa * aggs.naggs;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (mask_words && !((mask_words[i >> 6] >> (i & 63)) & 1)) continue;
    const u64 h = hash_keys_row(keys, i);
    u64 slot = h & cap_mask;
    int64_t probes = 0;
    u64* srec = nullptr;
    while (true) {
      u64* cand = slot_data + slot * rec;
      u64 cur = __hip_atomic_load(cand, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
      if (cur == 0) {
        u64 old = atomicCAS(cand, 0ull, (u64)i + 1);
        if (old == 0) { srec = cand; break; }
        cur = old;
      }
      if (cur != 0 && keys_equal_rows(keys, (int64_t)cur - 1, i)) {
        srec = cand;
        break;
      }
      slot = (slot + 1) & cap_mask;
      if (++probes > (int64_t)cap_mask) {  // table full
        atomicExch(err_flag, 1);
        return;
      }
    }
    atomicAdd(&srec[1], 1ull);
    for (int a = 0; a < aggs.naggs; ++a) {
      u64* base = srec + 2 + wpa * a;
      // SQL aggregate null semantics: a NULL value contributes nothing
      if (!bit_valid(aggs.a[a].valid, i)) continue;
      if (aggs.vmode) atomicAdd(&base[2], 1ull);
      switch (aggs.a[a].op) {
        case BG_AGG_OP_SUM_DEC128: {
          const ulong2 v =
              reinterpret_cast<const ulong2*>(aggs.a[a].data)[i];
          atomic_add_i128(base, base + 1, make_i128(v.x, (i64)v.y));
          break;
        }
        case BG_AGG_OP_SUM_I64: {
          const i64 v = reinterpret_cast<const int64_t*>(aggs.a[a].data)[i];
          // exact i64 sum in two's complement (wrap == i64 semantics);
          // keep the i128 carry so large sums stay exact at scale
          atomic_add_i128(base, base + 1, (i128)v);
          break;
        }
        case BG_AGG_OP_MAX_I64: {
          const u64 v = (u64) reinterpret_cast<const int64_t*>(
                            aggs.a[a].data)[i] ^ 0x8000000000000000ull;
          atomicMax(base, v);
          break;
        }
        case BG_AGG_OP_MIN_I64: {
          const u64 v = ~((u64) reinterpret_cast<const int64_t*>(
                              aggs.a[a].data)[i] ^ 0x8000000000000000ull);
          atomicMax(base, v);
          break;
        }
        case BG_AGG_OP_SUM_F64: {
          const double v = reinterpret_cast<const double*>(aggs.a[a].data)[i];
          atomicAdd(reinterpret_cast<double*>(base), v);
          break;
        }
        case BG_AGG_OP_MAX_F64: {
          // IEEE-754 totally-ordered u64 transform (sign-magnitude flip):
          // monotone for all finite values and infs, as the reference's
          // min_max.rs float compare is
          const u64 bits = (u64) reinterpret_cast<const int64_t*>(
                               aggs.a[a].data)[i];
          const u64 v = (bits & 0x8000000000000000ull)
                            ? ~bits
                            : bits ^ 0x8000000000000000ull;
          atomicMax(base, v);
          break;
        }
        case BG_AGG_OP_MIN_F64: {
          const u64 bits = (u64) reinterpret_cast<const int64_t*>(
                               aggs.a[a].data)[i];
          const u64 v = (bits & 0x8000000000000000ull)
                            ? ~bits
                            : bits ^ 0x8000000000000000ull;
          atomicMax(base, ~v);
          break;
        }
        case BG_AGG_OP_MAX_I32: {
          const u64 v = (u64)(i64) reinterpret_cast<const int32_t*>(
                            aggs.a[a].data)[i] ^ 0x8000000000000000ull;
          atomicMax(base, v);
          break;
        }
        case BG_AGG_OP_MIN_I32: {
          const u64 v = ~((u64)(i64) reinterpret_cast<const int32_t*>(
                              aggs.a[a].data)[i] ^ 0x8000000000000000ull);
          atomicMax(base, v);
          break;
        }
        case BG_AGG_OP_MIN_ROW:
        case BG_AGG_OP_MAX_ROW:
          agg_row_update<__HIP_MEMORY_SCOPE_AGENT>(base, (u64)i + 1,
                                                   aggs.a[a]);
          break;
        default:
          break;
      }
    }
  }
}

// Low-cardinality fast path (q1-class: a handful of groups over hundreds
// of millions of rows): the global open table serialises every row on a
// few device-scope atomic lines (measured 21 s for SF100 q1 through the
// generic path).  Each BLOCK accumulates into its own LDS table with the
// same record layout, then flushes occupied slots into the global table
// with op-aware atomic merges.  If a block overflows its LDS capacity it
// aborts the whole launch with err=2 (no flush) and the host falls back
// to the global-table kernel on a zeroed table.
__global__ void k_hashagg_lds(KeyArgs keys, AggArgs aggs,
                              const u64* mask_words, int64_t n,
                              u64 lds_cap_mask, u64 gcap_mask,
                              u64* slot_data, int* err_flag) {
  extern __shared__ u64 lt[];
  const int wpa = 2 + aggs.vmode;
  const int rec = 2 + wpa * aggs.naggs;
  const int64_t lds_cap = (int64_t)lds_cap_mask + 1;
  for (int64_t w = threadIdx.x; w < lds_cap * rec; w += blockDim.x) lt[w] = 0;
  __shared__ int overflow;
  if (threadIdx.x == 0) overflow = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (__hip_atomic_load(&overflow, __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_WORKGROUP))
      break;
    if (mask_words && !((mask_words[i >> 6] >> (i & 63)) & 1)) continue;
    const u64 h = hash_keys_row(keys, i);
    u64 slot = h & lds_cap_mask;
    int64_t probes = 0;
    u64* srec = nullptr;
    while (true) {
      u64* cand = lt + slot * rec;
      u64 cur = __hip_atomic_load(cand, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_WORKGROUP);
      if (cur == 0) {
        u64 old = atomicCAS((unsigned long long*)cand, 0ull, (u64)i + 1);
        if (old == 0) { srec = cand; break; }
        cur = old;
      }
      if (cur != 0 && keys_equal_rows(keys, (int64_t)cur - 1, i)) {
        srec = cand;
        break;
      }
      slot = (slot + 1) & lds_cap_mask;
      if (++probes > (int64_t)lds_cap_mask) {
        atomicExch(&overflow, 1);
        atomicExch(err_flag, 2);
        srec = nullptr;
        break;
      }
    }
    if (!srec) break;
    atomicAdd((unsigned long long*)&srec[1], 1ull);
    for (int a = 0; a < aggs.naggs; ++a) {
      u64* base = srec + 2 + wpa * a;
      if (!bit_valid(aggs.a[a].valid, i)) continue;
      if (aggs.vmode) atomicAdd((unsigned long long*)&base[2], 1ull);
      switch (aggs.a[a].op) {
        case BG_AGG_OP_SUM_DEC128: {
          const ulong2 v =
              reinterpret_cast<const ulong2*>(aggs.a[a].data)[i];
          atomic_add_i128(base, base + 1, make_i128(v.x, (i64)v.y));
          break;
        }
        case BG_AGG_OP_SUM_I64: {
          const i64 v = reinterpret_cast<const int64_t*>(aggs.a[a].data)[i];
          atomic_add_i128(base, base + 1, (i128)v);
          break;
        }
        case BG_AGG_OP_MAX_I64: {
          const u64 v = (u64) reinterpret_cast<const int64_t*>(
                            aggs.a[a].data)[i] ^ 0x8000000000000000ull;
          atomicMax((unsigned long long*)base, v);
          break;
        }
        case BG_AGG_OP_MIN_I64: {
          const u64 v = ~((u64) reinterpret_cast<const int64_t*>(
                              aggs.a[a].data)[i] ^ 0x8000000000000000ull);
          atomicMax((unsigned long long*)base, v);
          break;
        }
        case BG_AGG_OP_SUM_F64: {
          const double v = reinterpret_cast<const double*>(aggs.a[a].data)[i];
          atomicAdd(reinterpret_cast<double*>(base), v);
          break;
        }
        case BG_AGG_OP_MAX_F64: {
          const u64 bits = (u64) reinterpret_cast<const int64_t*>(
                               aggs.a[a].data)[i];
          const u64 v = (bits & 0x8000000000000000ull)
                            ? ~bits
                            : bits ^ 0x8000000000000000ull;
          atomicMax((unsigned long long*)base, v);
          break;
        }
        case BG_AGG_OP_MIN_F64: {
          const u64 bits = (u64) reinterpret_cast<const int64_t*>(
                               aggs.a[a].data)[i];
          const u64 v = (bits & 0x8000000000000000ull)
                            ? ~bits
                            : bits ^ 0x8000000000000000ull;
          atomicMax((unsigned long long*)base, ~v);
          break;
        }
        case BG_AGG_OP_MAX_I32: {
          const u64 v = (u64)(i64) reinterpret_cast<const int32_t*>(
                            aggs.a[a].data)[i] ^ 0x8000000000000000ull;
          atomicMax((unsigned long long*)base, v);
          break;
        }
        case BG_AGG_OP_MIN_I32: {
          const u64 v = ~((u64)(i64) reinterpret_cast<const int32_t*>(
                              aggs.a[a].data)[i] ^ 0x8000000000000000ull);
          atomicMax((unsigned long long*)base, v);
          break;
        }
        case BG_AGG_OP_MIN_ROW:
        case BG_AGG_OP_MAX_ROW:
          // row numbers are global, so the block's winner stays
          // meaningful in the flush below
          agg_row_update<__HIP_MEMORY_SCOPE_WORKGROUP>(base, (u64)i + 1,
                                                       aggs.a[a]);
          break;
        default:
          break;
      }
    }
  }
  __syncthreads();
  if (overflow) return;
  // flush: merge each occupied LDS record into the global table
  for (int64_t s = threadIdx.x; s < lds_cap; s += blockDim.x) {
    u64* lrec = lt + s * rec;
    const u64 claim = lrec[0];
    if (!claim) continue;
    const int64_t row = (int64_t)claim - 1;
    const u64 h = hash_keys_row(keys, row);
    u64 slot = h & gcap_mask;
    int64_t probes = 0;
    u64* grec = nullptr;
    while (true) {
      u64* cand = slot_data + slot * rec;
      u64 cur = __hip_atomic_load(cand, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
      if (cur == 0) {
        u64 old = atomicCAS(cand, 0ull, claim);
        if (old == 0) { grec = cand; break; }
        cur = old;
      }
      if (cur != 0 && keys_equal_rows(keys, (int64_t)cur - 1, row)) {
        grec = cand;
        break;
      }
      slot = (slot + 1) & gcap_mask;
      if (++probes > (int64_t)gcap_mask) {
        atomicExch(err_flag, 1);
        return;
      }
    }
    atomicAdd(&grec[1], lrec[1]);
    for (int a = 0; a < aggs.naggs; ++a) {
      u64* g = grec + 2 + wpa * a;
      const u64* l = lrec + 2 + wpa * a;
      if (aggs.vmode) atomicAdd(&g[2], l[2]);
      switch (aggs.a[a].op) {
        case BG_AGG_OP_SUM_DEC128:
        case BG_AGG_OP_SUM_I64:
          atomic_add_i128(g, g + 1, make_i128(l[0], (i64)l[1]));
          break;
        case BG_AGG_OP_MAX_I64:
        case BG_AGG_OP_MIN_I64:
        case BG_AGG_OP_MAX_F64:
        case BG_AGG_OP_MIN_F64:
        case BG_AGG_OP_MAX_I32:
        case BG_AGG_OP_MIN_I32:
          atomicMax(g, l[0]);
          break;
        case BG_AGG_OP_MIN_ROW:
        case BG_AGG_OP_MAX_ROW:
          // the block's winner is the candidate (0: no non-NULL row here)
          if (l[0])
            agg_row_update<__HIP_MEMORY_SCOPE_AGENT>(g, l[0], aggs.a[a]);
          break;
        case BG_AGG_OP_SUM_F64: {
          double v;
          memcpy(&v, &l[0], 8);
          atomicAdd(reinterpret_cast<double*>(g), v);
          break;
        }
        default:
          break;
      }
    }
  }
}

// occupancy bitmask over slots (feeds the stable compaction)

__global__ void k_slot_occupancy(const u64* slot_data, int rec, int64_t cap,
                                 u64* mask_words) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  const int64_t nwords = (cap + 63) / 64;
  for (int64_t w = wave_global; w < nwords; w += nwaves) {
    const int64_t s = w * BG_WAVE + lane_id();
    const bool occ = s < cap && slot_data[(u64)s * rec] != 0;
    u64 m = __ballot(occ);
    if (lane_id() == 0) mask_words[w] = m;
  }
}

// gather group outputs: for dense group g = 0..ngroups-1 with slot index
// sidx[g]: first_row[g], counts_out[g], acc_out[g*naggs*2 ..]
__global__ void k_hashagg_gather(const uint32_t* sidx, int64_t ngroups,
                                 const u64* slot_data, int naggs, int vmode,
                                 uint32_t* first_row, u64* counts_out,
                                 u64* acc_out, u64* nncnt_out) {
  const int wpa = 2 + vmode;
  const int rec = 2 + wpa * naggs;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups;
       g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = sidx[g];
    const u64* srec = slot_data + (u64)s * rec;
    first_row[g] = (uint32_t)(srec[0] - 1);
    counts_out[g] = srec[1];
    for (int a = 0; a < naggs; ++a) {
      acc_out[((u64)g * naggs + a) * 2] = srec[2 + wpa * a];
      acc_out[((u64)g * naggs + a) * 2 + 1] = srec[2 + wpa * a + 1];
      if (vmode && nncnt_out)
        nncnt_out[(u64)g * naggs + a] = srec[2 + wpa * a + 2];
    }
  }
}

static int hashagg_impl(const bg_column* key_cols, int32_t nkeys,
                        const bg_column* agg_cols, const int32_t* agg_ops,
                        int32_t naggs, const uint8_t* d_mask, int64_t n,
                        int64_t max_groups, uint32_t* d_first_row,
                        uint8_t* d_acc_out, int64_t* d_counts_out,
                        int64_t* d_nncnt_out, int64_t* out_ngroups) {
  REQUIRE_INIT();
  const int vmode = d_nncnt_out ? 1 : 0;
  if (nkeys <= 0 || nkeys > BG_MAX_KEYS)
    return set_err(BG_ERR_INVALID, "nkeys out of range [1,4]");
  if (naggs < 0 || naggs > BG_MAX_AGGS)
    return set_err(BG_ERR_INVALID, "naggs out of range [0,8]");
  // the ops that read their column by dtype (before any device allocation)
  for (int i = 0; i < naggs; ++i) {
    const int32_t op = agg_ops[i], dt = agg_cols[i].dtype;
    if ((op == BG_AGG_OP_MIN_ROW || op == BG_AGG_OP_MAX_ROW) &&
        dt != BG_DT_DECIMAL128 && dt != BG_DT_UTF8)
      return set_err(BG_ERR_UNSUPPORTED,
                     "bg_hashagg: MIN_ROW/MAX_ROW take Decimal128 or Utf8");
    if ((op == BG_AGG_OP_MIN_ROW || op == BG_AGG_OP_MAX_ROW) &&
        dt == BG_DT_UTF8 && !agg_cols[i].d_offsets)
      return set_err(BG_ERR_INVALID,
                     "bg_hashagg: Utf8 aggregate column without offsets");
    if ((op == BG_AGG_OP_MIN_I32 || op == BG_AGG_OP_MAX_I32) &&
        dt != BG_DT_INT32 && dt != BG_DT_DATE32)
      return set_err(BG_ERR_UNSUPPORTED,
                     "bg_hashagg: MIN_I32/MAX_I32 take Int32 or Date32");
  }
  KeyArgs keys{};
  keys.nkeys = nkeys;
  for (int i = 0; i < nkeys; ++i) {
    keys.k[i].data = key_cols[i].d_data;
    keys.k[i].valid = key_cols[i].d_validity;
    keys.k[i].offsets = key_cols[i].d_offsets;
    keys.k[i].dtype = key_cols[i].dtype;
  }
  AggArgs aggs{};
  aggs.naggs = naggs;
  aggs.vmode = vmode;
  for (int i = 0; i < naggs; ++i) {
    aggs.a[i].data = agg_cols[i].d_data;
    aggs.a[i].valid = agg_cols[i].d_validity;
    aggs.a[i].offsets = agg_cols[i].d_offsets;
    aggs.a[i].op = agg_ops[i];
    aggs.a[i].dtype = agg_cols[i].dtype;
  }
  u64 cap = 8;
  while (cap < (u64)(max_groups * 2)) cap <<= 1;
  const int rec = 2 + (2 + vmode) * naggs;
  DevBuf<u64> slot_data;
  DevBuf<int> err_flag;
  HIP_TRY(slot_data.alloc(cap * rec));
  HIP_TRY(err_flag.alloc(1));
  HIP_TRY(hipMemset(slot_data, 0, sizeof(u64) * cap * rec));
  HIP_TRY(hipMemset(err_flag, 0, sizeof(int)));

  int blocks = grid_for(n);
  // low-cardinality first attempt: per-block LDS tables (48 KB budget).
  // Overflow (more groups than the LDS capacity) aborts with err=2 and
  // we fall back to the global-table kernel on a zeroed table.
  u64 lds_cap = 8;
  while (lds_cap * 2 * (u64)rec * 8 <= 48 * 1024 && lds_cap < 4096)
    lds_cap <<= 1;
  const bool try_lds = lds_cap >= 64 && n >= (1 << 16);
  EventPair ev;
  HIP_TRY(ev.create());
  HIP_TRY(hipEventRecord(ev.ev0, 0));
  bool lds_done = false;
  if (try_lds) {
    hipLaunchKernelGGL(k_hashagg_lds, dim3(blocks), dim3(BG_BLOCK),
                       lds_cap * (u64)rec * 8, 0, keys, aggs,
                       reinterpret_cast<const u64*>(d_mask), n, lds_cap - 1,
                       cap - 1, slot_data, err_flag);
    HIP_TRY(hipGetLastError());
    int lerr = 0;
    HIP_TRY(hipMemcpy(&lerr, err_flag, sizeof(int), hipMemcpyDeviceToHost));
    if (lerr == 2) {  // LDS overflow: clean retry on the global path
      HIP_TRY(hipMemset(slot_data, 0, sizeof(u64) * cap * rec));
      HIP_TRY(hipMemset(err_flag, 0, sizeof(int)));
    } else {
      lds_done = true;
    }
  }
  if (!lds_done)
    hipLaunchKernelGGL(k_hashagg, dim3(blocks), dim3(BG_BLOCK), 0, 0, keys,
                       aggs, reinterpret_cast<const u64*>(d_mask), n, cap - 1,
                       slot_data, err_flag);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ev.ev1, 0));
  HIP_TRY(hipEventSynchronize(ev.ev1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.ev0, ev.ev1));
  g_last_kernel_ms = (double)ms;

  int err = 0;
  HIP_TRY(hipMemcpy(&err, err_flag, sizeof(int), hipMemcpyDeviceToHost));
  if (err)
    return set_err(BG_ERR_INVALID, "bg_hashagg: table full (raise max_groups)");

  // compact occupied slots (ascending slot order — deterministic for a
  // fixed capacity) using the occupancy mask + stable compaction
  const int64_t nwords = ((int64_t)cap + 63) / 64;
  DevBuf<u64> occ_mask;
  DevBuf<uint32_t> sidx;
  HIP_TRY(occ_mask.alloc(nwords));
  HIP_TRY(sidx.alloc(cap));
  int oblocks = grid_for(nwords * BG_WAVE);
  hipLaunchKernelGGL(k_slot_occupancy, dim3(oblocks), dim3(BG_BLOCK), 0, 0,
                     slot_data, rec, (int64_t)cap, occ_mask);
  int64_t ngroups = 0;
  int rc = bg_mask_to_indices(reinterpret_cast<const uint8_t*>(occ_mask.get()),
                              (int64_t)cap, sidx, &ngroups);
  if (rc != BG_OK) return rc;
  if (ngroups > max_groups)
    // the open table (capacity 2*max_groups rounded up) absorbed more
    // distinct groups than the caller's OUTPUT buffers hold
    return set_err(BG_ERR_INVALID,
                   "bg_hashagg: table full (raise max_groups — more groups "
                   "than output capacity)");

  int gblocks = grid_for(ngroups);
  hipLaunchKernelGGL(k_hashagg_gather, dim3(gblocks), dim3(BG_BLOCK), 0, 0,
                     sidx, ngroups, slot_data, naggs, vmode, d_first_row,
                     reinterpret_cast<u64*>(d_counts_out),
                     reinterpret_cast<u64*>(d_acc_out),
                     reinterpret_cast<u64*>(d_nncnt_out));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  *out_ngroups = ngroups;
  return BG_OK;
}

extern "C" int bg_hashagg(const bg_column* key_cols, int32_t nkeys,
                          const bg_column* agg_cols, const int32_t* agg_ops,
                          int32_t naggs, const uint8_t* d_mask, int64_t n,
                          int64_t max_groups, uint32_t* d_first_row,
                          uint8_t* d_acc_out, int64_t* d_counts_out,
                          int64_t* out_ngroups) {
  return hashagg_impl(key_cols, nkeys, agg_cols, agg_ops, naggs, d_mask, n,
                      max_groups, d_first_row, d_acc_out, d_counts_out,
                      nullptr, out_ngroups);
}

/* As bg_hashagg but also reports the per-(group, aggregate) NON-NULL input
 * count (d_nncnt_out, ngroups*naggs i64): SQL reports SUM/MIN/MAX of a
 * group whose inputs were all NULL as NULL, which the accumulator value
 * alone cannot encode.  Mirrors the reference's accumulators
 * (datafusion/physical-expr aggregates) returning Option-valued state. */
extern "C" int bg_hashagg2(const bg_column* key_cols, int32_t nkeys,
                           const bg_column* agg_cols, const int32_t* agg_ops,
                           int32_t naggs, const uint8_t* d_mask, int64_t n,
                           int64_t max_groups, uint32_t* d_first_row,
                           uint8_t* d_acc_out, int64_t* d_counts_out,
                           int64_t* d_nncnt_out, int64_t* out_ngroups) {
  return hashagg_impl(key_cols, nkeys, agg_cols, agg_ops, naggs, d_mask, n,
                      max_groups, d_first_row, d_acc_out, d_counts_out,
                      d_nncnt_out, out_ngroups);
}

// ---------------------------------------------------------------------------
// ProjectionExec expression subset: Decimal128 binary arithmetic
// (DataFusion 55 expression eval on the hot path — SURVEY.md §1 "expression
// eval"; exact i128, Arrow decimal scale handling is the planner's concern).
// ops: 0 a*b, 1 a+b, 2 a-b, 3 lit-a, 4 a*lit, 5 a+lit
// ---------------------------------------------------------------------------
__global__ void k_project_dec128(int op, const ulong2* a, const ulong2* b,
                                 i128 lit, int64_t n, ulong2* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const ulong2 av = a[i];
    const i128 x = make_i128(av.x, (i64)av.y);
    i128 r;
    switch (op) {
      case 0: { const ulong2 bv = b[i]; r = x * make_i128(bv.x, (i64)bv.y); break; }
      case 1: { const ulong2 bv = b[i]; r = x + make_i128(bv.x, (i64)bv.y); break; }
      case 2: { const ulong2 bv = b[i]; r = x - make_i128(bv.x, (i64)bv.y); break; }
      case 3: r = lit - x; break;
      case 4: r = x * lit; break;
      case 5: r = x + lit; break;
      default: r = 0;
    }
    ulong2 o;
    o.x = (u64)(u128)r;
    o.y = (u64)((u128)r >> 64);
    out[i] = o;
  }
}

extern "C" int bg_project_dec128(int32_t op, const bg_column* a,
                                 const bg_column* b, int64_t lit_lo,
                                 int64_t lit_hi, int64_t n, void* d_out) {
  REQUIRE_INIT();
  if (op <= 2 && b == nullptr)
    return set_err(BG_ERR_INVALID, "binary op needs column b");
  int blocks = grid_for(n);
  const i128 lit = ((i128)lit_hi << 64) | (i128)(u128)(u64)lit_lo;
  hipLaunchKernelGGL(k_project_dec128, dim3(blocks), dim3(BG_BLOCK), 0, 0, op,
                     (const ulong2*)a->d_data,
                     b ? (const ulong2*)b->d_data : nullptr, lit, n,
                     (ulong2*)d_out);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---------------------------------------------------------------------------
// SortExec: stable LSD radix sort of row permutations,
// built on the same stable 256-way split that powers the hash repartition
// (each pass: digit extract -> k_part_hist/scan/k_part_scatter -> permute).
// Order-preserving key transform: i64 -> u64 (sign flip), descending -> ~u.
// Stability makes multi-column ORDER BY composable: sort by the LAST key
// first, then each earlier key (classic LSD over columns), and makes the
// permutation bit-exact against a stable argsort oracle.
// ---------------------------------------------------------------------------
__global__ void k_sort_digit_seq(const u64* keyu_cur, int64_t n, int shift,
                                 uint32_t* pids) {
  // keys are kept in CURRENT permutation order, so the digit read is a
  // sequential stream (the gather-by-perm variant random-reads the key
  // array and pays k-fold line amplification)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    pids[i] = (uint32_t)((keyu_cur[i] >> shift) & 0xffu);
}

__global__ void k_key_transform_i64(const int64_t* keys,
                                    const uint8_t* valid, int64_t n,
                                    int descending, u64* keyu) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (!bit_valid(valid, i)) { keyu[i] = 0; continue; }  // stable nulls
    u64 u = (u64)keys[i] ^ 0x8000000000000000ull;
    keyu[i] = descending ? ~u : u;
  }
}

// Float64 ORDER BY: IEEE-754 total-order transform (sign-magnitude
// flip — negatives bit-inverted, positives sign-flipped; same monotone
// map the MIN/MAX aggregates use)
__global__ void k_key_transform_f64(const int64_t* keys,
                                    const uint8_t* valid, int64_t n,
                                    int descending, u64* keyu) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (!bit_valid(valid, i)) { keyu[i] = 0; continue; }
    const u64 bits = (u64)keys[i];
    const u64 u = (bits & 0x8000000000000000ull)
                      ? ~bits
                      : bits ^ 0x8000000000000000ull;
    keyu[i] = descending ? ~u : u;
  }
}

__global__ void k_key_transform_i32(const int32_t* keys,
                                    const uint8_t* valid, int64_t n,
                                    int descending, u64* keyu) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (!bit_valid(valid, i)) { keyu[i] = 0; continue; }
    u64 u = (u64)((uint32_t)keys[i] ^ 0x80000000u);
    keyu[i] = descending ? (~u & 0xffffffffull) : u;
  }
}

// Decimal128 -> order-preserving (hi, lo) u64 pair (sign-flip the high word)
__global__ void k_key_transform_dec128(const ulong2* keys,
                                       const uint8_t* valid, int64_t n,
                                       int descending, u64* key_lo,
                                       u64* key_hi) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (!bit_valid(valid, i)) {
      key_lo[i] = 0;
      key_hi[i] = 0;
      continue;
    }
    const ulong2 v = keys[i];
    u64 lo = v.x;
    u64 hi = v.y ^ 0x8000000000000000ull;
    if (descending) { lo = ~lo; hi = ~hi; }
    key_lo[i] = lo;
    key_hi[i] = hi;
  }
}

// apply the initial permutation (or identity) to a key stream
__global__ void k_permute_u64(const u64* src, const uint32_t* perm, int64_t n,
                              u64* dst) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = src[perm[i]];
}

__global__ void k_iota_u32(uint32_t* p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = (uint32_t)i;
}

__device__ __forceinline__ u64 keyu_load(const u64* p, int64_t i) {
  return __builtin_nontemporal_load(&p[i]);
}
__device__ __forceinline__ u64 klo_or_hi(u64 lo, u64 hi, int shift,
                                         int has_hi) {
  // shift in [0,64) addresses the lo word; [64,128) the hi word
  return shift < 64 ? (lo >> shift) : (has_hi ? (hi >> (shift - 64)) : 0);
}
__device__ __forceinline__ uint32_t bcast_from_lane(uint32_t v, int lane_src) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, lane_src);
}

// ---------------------------------------------------------------------------
// Fused radix pass: digit extraction folded into histogram and scatter, and
// the scatter MATERIALISES the next key/perm orders directly (no pids
// array, no separate rank+apply passes) — per pass: read keys twice,
// write keys+perm once, vs the generic split's 5 streams.
// ---------------------------------------------------------------------------
__global__ void k_radix_hist(const u64* keyu, int64_t n, int shift,
                             u64* hist, int64_t nchunks) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  uint32_t* cnt = reinterpret_cast<uint32_t*>(smem_raw);
  const int wave_in_block = threadIdx.x / BG_WAVE;
  uint32_t* my = cnt + (size_t)wave_in_block * 256;
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t c = wave_global; c < nchunks; c += nwaves) {
    for (uint32_t p = lane_id(); p < 256; p += BG_WAVE) my[p] = 0;
    __builtin_amdgcn_wave_barrier();
    const int64_t r0 = c * PS_ROWS_PER_WAVE;
    const int64_t r1 = min(r0 + (int64_t)PS_ROWS_PER_WAVE, n);
    for (int64_t r = r0 + lane_id(); r < r1; r += BG_WAVE)
      atomicAdd(&my[(uint32_t)((keyu_load(keyu, r) >> shift) & 0xffu)], 1u);
    __builtin_amdgcn_wave_barrier();
    for (uint32_t p = lane_id(); p < 256; p += BG_WAVE)
      hist[(int64_t)p * nchunks + c] = my[p];
  }
}

// nwords: 1 or 2 key words; scatters key word(s) and perm into next order
__global__ void k_radix_scatter(const u64* key_lo, const u64* key_hi,
                                const uint32_t* perm, int64_t n, int shift,
                                const i64* start, int64_t nchunks,
                                u64* out_lo, u64* out_hi, uint32_t* out_perm,
                                int has_hi) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  i64* cur = reinterpret_cast<i64*>(smem_raw);
  const int wave_in_block = threadIdx.x / BG_WAVE;
  i64* my = cur + (size_t)wave_in_block * 256;
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  const int lane = lane_id();
  for (int64_t c = wave_global; c < nchunks; c += nwaves) {
    for (uint32_t p = lane; p < 256; p += BG_WAVE)
      my[p] = start[(int64_t)p * nchunks + c];
    __builtin_amdgcn_wave_barrier();
    const int64_t r0 = c * PS_ROWS_PER_WAVE;
    const int64_t r1 = min(r0 + (int64_t)PS_ROWS_PER_WAVE, n);
    for (int64_t rb = r0; rb < r1; rb += BG_WAVE) {
      const int64_t r = rb + lane;
      const bool active = r < r1;
      u64 klo = 0, khi = 0;
      uint32_t pm = 0;
      uint32_t pid = 0xffffffffu;
      if (active) {
        klo = keyu_load(key_lo, r);
        if (has_hi) khi = keyu_load(key_hi, r);
        pm = perm[r];
        pid = (uint32_t)((klo_or_hi(klo, khi, shift, has_hi)) & 0xffu);
      }
      // ballot-bit multi-split: 8 ballots give each lane the mask of
      // active lanes sharing its digit; rank = popc(lower same-digit
      // lanes) — stable, no serialized per-digit loop.
      const u64 act = __ballot(active);
      u64 same = act;
      for (int b = 0; b < 8; ++b) {
        const u64 bb = __ballot(((pid >> b) & 1u) != 0u);
        same &= ((pid >> b) & 1u) ? bb : ~bb;
      }
      if (active) {
        const u64 lower = same & ((1ull << lane) - 1);
        const i64 base = my[pid];
        const i64 pos = base + __popcll(lower);
        out_lo[pos] = klo;
        if (has_hi) out_hi[pos] = khi;
        out_perm[pos] = pm;
        __builtin_amdgcn_wave_barrier();
        if (lower == 0) my[pid] = base + __popcll(same);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// One block, 256 lanes: lane d sums hist row d over chunks; if any digit
// owns ALL n rows the pass is an identity permutation and can be skipped.
__global__ void k_hist_trivial(const u64* hist, int64_t nchunks, int64_t n,
                               int* flag) {
  // block d reduces digit row d; 256 lanes stride the chunks
  __shared__ u64 part[256];
  const int d = blockIdx.x;
  u64 t = 0;
  for (int64_t c = threadIdx.x; c < nchunks; c += blockDim.x)
    t += hist[(int64_t)d * nchunks + c];
  part[threadIdx.x] = t;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0 && (int64_t)part[0] == n) *flag = 1;
}

// Stable radix passes over one or two u64 key words held in CURRENT
// permutation order, via the fused digit+hist and digit+scatter+materialise
// kernels above (no pids array, no separate rank/apply passes).
// d_key_words are the caller's OWNERS: each scatter pass swaps them with
// this function's spare buffers, so on return the caller holds whichever
// buffers carry the sorted keys and the spares are released here — every
// buffer exactly once, whoever ends up holding it.
static int radix_sort_passes(DevBuf<u64> d_key_words[2], int nwords,
                             int64_t n, uint32_t* d_perm,
                             int npasses_per_word) {
  const int64_t nchunks = (n + PS_ROWS_PER_WAVE - 1) / PS_ROWS_PER_WAVE;
  const int64_t hist_len = 256 * (nchunks ? nchunks : 1);
  DevBuf<u64> d_hist;
  DevBuf<i64> d_start;
  DevBuf<u64> d_nxt[2];
  DevBuf<uint32_t> d_nxtperm;  // the other half of the perm ping-pong
  HIP_TRY(d_hist.alloc(hist_len));
  HIP_TRY(d_start.alloc(hist_len));
  HIP_TRY(d_nxtperm.alloc(n));
  DevBuf<int> d_flag;
  HIP_TRY(d_flag.alloc(1));
  for (int w = 0; w < nwords; ++w) HIP_TRY(d_nxt[w].alloc(n));
  const int waves_per_block = BG_BLOCK / BG_WAVE;
  const size_t lds_hist = (size_t)waves_per_block * 256 * sizeof(uint32_t);
  const size_t lds_scat = (size_t)waves_per_block * 256 * sizeof(i64);
  int blocks = grid_for(nchunks, 1);
  int rc = BG_OK;
  const int total_passes = npasses_per_word * nwords;
  uint32_t* perm_cur = d_perm;
  uint32_t* perm_nxt = d_nxtperm;
  for (int p = 0; p < total_passes && rc == BG_OK; ++p) {
    const int word = p / npasses_per_word;  // lo word first (LSD)
    const int shift = 8 * (p % npasses_per_word) + 64 * word;
    const u64* digit_src = d_key_words[word];
    hipLaunchKernelGGL(k_radix_hist, dim3(blocks), dim3(BG_BLOCK), lds_hist,
                       0, digit_src, n, 8 * (p % npasses_per_word), d_hist,
                       nchunks);
    // constant-digit pass = identity permutation: skip the scatter.  TPC-H
    // keys occupy < 2^31 so half the i64 passes (and ~9/16 Decimal128
    // passes) vanish.
    {
      hipError_t e = hipMemsetAsync(d_flag, 0, sizeof(int), 0);
      if (e != hipSuccess) { rc = set_hip_err(e, "flag clear"); break; }
      hipLaunchKernelGGL(k_hist_trivial, dim3(256), dim3(256), 0, 0, d_hist,
                         nchunks, n, d_flag);
      int h_flag = 0;
      e = hipMemcpy(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost);
      if (e != hipSuccess) { rc = set_hip_err(e, "flag copy"); break; }
      if (h_flag) continue;
    }
    rc = scan_exclusive_i64(d_hist, hist_len, d_start, nullptr);
    if (rc != BG_OK) break;
    // scatter the REMAINING words (word..nwords-1) + perm into next order
    const u64* klo = d_key_words[word];
    const u64* khi = (nwords == 2 && word == 0) ? d_key_words[1] : nullptr;
    u64* olo = d_nxt[word];
    u64* ohi = (nwords == 2 && word == 0) ? d_nxt[1] : nullptr;
    hipLaunchKernelGGL(k_radix_scatter, dim3(blocks), dim3(BG_BLOCK),
                       lds_scat, 0, klo, khi, perm_cur, n,
                       8 * (p % npasses_per_word), d_start, nchunks, olo, ohi,
                       perm_nxt, khi ? 1 : 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rc = set_hip_err(e, "radix scatter"); break; }
    // ping-pong
    d_key_words[word].swap(d_nxt[word]);
    if (khi) d_key_words[1].swap(d_nxt[1]);
    uint32_t* tp = perm_cur;
    perm_cur = perm_nxt;
    perm_nxt = tp;
  }
  if (rc == BG_OK && perm_cur != d_perm) {
    hipError_t e = hipMemcpyAsync(d_perm, perm_cur, sizeof(uint32_t) * n,
                                  hipMemcpyDeviceToDevice, 0);
    if (e != hipSuccess) rc = set_hip_err(e, "perm copy");
  }
  return rc;
}

// Utf8 sort keys: LSD radix over 8-byte big-endian chunks with a final
// length tiebreak chunk sorted FIRST — exact memcmp-then-length order
// (DataFusion's Utf8 comparator semantics).  Keys are extracted in the
// CURRENT permutation order each chunk, so stability composes across
// chunks; constant-digit pass skipping eats the sparse high bytes.
__global__ void k_utf8_chunk_key(const uint8_t* data, const int32_t* offs,
                                 const uint8_t* valid, const uint32_t* perm,
                                 int64_t n,
                                 int64_t chunk /* -1 = length tiebreak */,
                                 int descending, u64* keyu) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t r = perm[i];
    if (!bit_valid(valid, (int64_t)r)) { keyu[i] = 0; continue; }
    const int32_t lo = offs[r];
    const int32_t len = offs[r + 1] - lo;
    u64 key;
    if (chunk < 0) {
      key = (u64)(uint32_t)len;
    } else {
      key = 0;
      const int64_t base = chunk * 8;
      for (int b = 0; b < 8; ++b) {
        const uint8_t c8 =
            (base + b < (int64_t)len) ? data[lo + base + b] : 0;
        key = (key << 8) | (u64)c8;
      }
    }
    keyu[i] = descending ? ~key : key;
  }
}

// null-ordering pass: the most significant criterion — valid rows get
// bit `valid_key`, null rows its complement (nulls_first: nulls -> 0)
__global__ void k_null_order_key(const uint8_t* valid, const uint32_t* perm,
                                 int64_t n, int nulls_first, u64* keyu) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const bool v = bit_valid(valid, (int64_t)perm[i]);
    keyu[i] = nulls_first ? (v ? 1 : 0) : (v ? 0 : 1);
  }
}

__global__ void k_utf8_maxlen(const int32_t* offs, int64_t n, int* out) {
  int m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t l = offs[i + 1] - offs[i];
    if (l > m) m = (int)l;
  }
  atomicMax(out, m);
}

/* Multi-column stable sort: keys applied LSD (last column first).  Each
 * column: INT64/INT32/DATE32/DECIMAL128/UTF8 (desc via bit-flip).
 * d_perm out: the row permutation realising the ORDER BY. */
static int sort_rows_impl(const bg_column* key_cols,
                          const int32_t* descending,
                          const int32_t* nulls_first, int32_t nkeys,
                          int64_t n, uint32_t* d_perm) {
  REQUIRE_INIT();
  if (nkeys <= 0 || nkeys > BG_MAX_KEYS)
    return set_err(BG_ERR_INVALID, "nkeys out of range [1,4]");
  int blocks = grid_for(n);
  hipLaunchKernelGGL(k_iota_u32, dim3(blocks), dim3(BG_BLOCK), 0, 0, d_perm, n);
  DevBuf<u64> d_keyu[2], d_keyperm[2];
  HIP_TRY(d_keyu[0].alloc(n));
  HIP_TRY(d_keyu[1].alloc(n));
  HIP_TRY(d_keyperm[0].alloc(n));
  HIP_TRY(d_keyperm[1].alloc(n));
  int rc = BG_OK;
  for (int c = nkeys - 1; c >= 0 && rc == BG_OK; --c) {
    int npasses, nwords;
    switch (key_cols[c].dtype) {
      case BG_DT_INT64:
        hipLaunchKernelGGL(k_key_transform_i64, dim3(blocks), dim3(BG_BLOCK),
                           0, 0, (const int64_t*)key_cols[c].d_data,
                           key_cols[c].d_validity, n,
                           descending[c], d_keyu[0].get());
        npasses = 8; nwords = 1;
        break;
      case BG_DT_FLOAT64:
        hipLaunchKernelGGL(k_key_transform_f64, dim3(blocks), dim3(BG_BLOCK),
                           0, 0, (const int64_t*)key_cols[c].d_data,
                           key_cols[c].d_validity, n,
                           descending[c], d_keyu[0].get());
        npasses = 8; nwords = 1;
        break;
      case BG_DT_INT32:
      case BG_DT_DATE32:
        hipLaunchKernelGGL(k_key_transform_i32, dim3(blocks), dim3(BG_BLOCK),
                           0, 0, (const int32_t*)key_cols[c].d_data,
                           key_cols[c].d_validity, n,
                           descending[c], d_keyu[0].get());
        npasses = 4; nwords = 1;
        break;
      case BG_DT_DECIMAL128:
        hipLaunchKernelGGL(k_key_transform_dec128, dim3(blocks),
                           dim3(BG_BLOCK), 0, 0,
                           (const ulong2*)key_cols[c].d_data,
                           key_cols[c].d_validity, n,
                           descending[c], d_keyu[0].get(),
                           d_keyu[1].get());
        npasses = 8; nwords = 2;
        break;
      case BG_DT_UTF8: {
        // LSD over 8-byte chunks: length tiebreak first, then byte
        // chunks from the string tail to the head; each chunk's keys are
        // extracted in the CURRENT perm order (no separate permute)
        const uint8_t* d_data = (const uint8_t*)key_cols[c].d_data;
        const int32_t* d_offs = key_cols[c].d_offsets;
        DevBuf<int> d_maxlen;
        HIP_TRY(d_maxlen.alloc(1));
        HIP_TRY(hipMemsetAsync(d_maxlen, 0, sizeof(int), 0));
        hipLaunchKernelGGL(k_utf8_maxlen, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                           d_offs, n, d_maxlen);
        int maxlen = 0;
        HIP_TRY(hipMemcpy(&maxlen, d_maxlen, sizeof(int),
                          hipMemcpyDeviceToHost));
        d_maxlen.reset();
        if (maxlen > (1 << 20))
          return set_err(BG_ERR_INVALID, "utf8 sort keys > 1 MiB");
        const int64_t nch = ((int64_t)maxlen + 7) / 8;
        for (int64_t j = -1; j < nch && rc == BG_OK; ++j) {
          const int64_t chunk = (j < 0) ? -1 : (nch - 1 - j);
          hipLaunchKernelGGL(k_utf8_chunk_key, dim3(blocks), dim3(BG_BLOCK),
                             0, 0, d_data, d_offs, key_cols[c].d_validity,
                             d_perm, n, chunk,
                             descending[c], d_keyperm[0].get());
          rc = radix_sort_passes(d_keyperm, 1, n, d_perm, 8);
        }
        if (rc == BG_OK && key_cols[c].d_validity) {
          hipLaunchKernelGGL(k_null_order_key, dim3(blocks), dim3(BG_BLOCK),
                             0, 0, key_cols[c].d_validity, d_perm, n,
                             nulls_first ? nulls_first[c] : descending[c],
                             d_keyperm[0].get());
          rc = radix_sort_passes(d_keyperm, 1, n, d_perm, 1);
        }
        continue;
      }
      default:
        rc = set_err(BG_ERR_UNSUPPORTED,
                     "sort keys: INT64/INT32/DATE32/DECIMAL128/UTF8/FLOAT64");
        continue;
    }
    // bring the key stream into the CURRENT permutation order once
    for (int w = 0; w < nwords; ++w)
      hipLaunchKernelGGL(k_permute_u64, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                         d_keyu[w].get(), d_perm, n, d_keyperm[w].get());
    rc = radix_sort_passes(d_keyperm, nwords, n, d_perm, npasses);
    if (rc == BG_OK && key_cols[c].d_validity) {
      // null-ordering pass — the MOST significant criterion for this
      // key: SQL default NULLS LAST for ASC, NULLS FIRST for DESC
      // unless the caller says otherwise (bg_sort_rows2)
      hipLaunchKernelGGL(k_null_order_key, dim3(blocks), dim3(BG_BLOCK),
                         0, 0, key_cols[c].d_validity, d_perm, n,
                         nulls_first ? nulls_first[c] : descending[c],
                         d_keyperm[0].get());
      rc = radix_sort_passes(d_keyperm, 1, n, d_perm, 1);
    }
  }
  if (rc == BG_OK) HIP_TRY(hipGetLastError());
  return rc;
}

extern "C" int bg_sort_rows(const bg_column* key_cols,
                            const int32_t* descending, int32_t nkeys,
                            int64_t n, uint32_t* d_perm) {
  return sort_rows_impl(key_cols, descending, nullptr, nkeys, n, d_perm);
}

/* As bg_sort_rows with explicit per-key null ordering (1 = NULLS FIRST);
 * bg_sort_rows defaults to the SQL convention (ASC -> NULLS LAST,
 * DESC -> NULLS FIRST).  Null rows sort as one stable group. */
extern "C" int bg_sort_rows2(const bg_column* key_cols,
                             const int32_t* descending,
                             const int32_t* nulls_first, int32_t nkeys,
                             int64_t n, uint32_t* d_perm) {
  return sort_rows_impl(key_cols, descending, nulls_first, nkeys, n, d_perm);
}


// ---------------------------------------------------------------------------
// SortMergeJoinExec (INNER, Int64 keys; SURVEY.md §8f row 2 second half —
// the reference's DEFAULT partitioned join, prefer_hash_join=false,
// core/src/extension.rs:850-858, every approved/q*.txt join stage).
// Both inputs sorted on the join key (bg_sort_rows upstream); each probe
// row binary-searches its build-side equal range -> exact per-row counts ->
// scan -> fill.  Output is FULLY ordered: probe-major, build ascending —
// stronger determinism than the hash join's chain order.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int64_t lower_bound_i64(const int64_t* a,
                                                   int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void k_merge_count(const int64_t* build_sorted, int64_t nb,
                              const int64_t* probe_sorted, int64_t np,
                              u64* counts, int64_t* lbs) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = probe_sorted[i];
    const int64_t lb = lower_bound_i64(build_sorted, nb, k);
    int64_t ub = lb;
    while (ub < nb && build_sorted[ub] == k) ++ub;  // runs are short in
    counts[i] = (u64)(ub - lb);                      // equi-join practice
    lbs[i] = lb;
  }
}

__global__ void k_merge_fill(const int64_t* build_sorted, int64_t nb,
                             int64_t np, const i64* offsets,
                             const int64_t* lbs, const u64* counts,
                             uint32_t* out_probe, uint32_t* out_build) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np;
       i += (int64_t)gridDim.x * blockDim.x) {
    i64 w = offsets[i];
    const int64_t lb = lbs[i];
    const int64_t c = (int64_t)counts[i];
    for (int64_t j = 0; j < c; ++j) {
      out_probe[w + j] = (uint32_t)i;
      out_build[w + j] = (uint32_t)(lb + j);
    }
  }
}

/* Inner merge join of two KEY-SORTED Int64 arrays.  Emits positions INTO
 * THE SORTED ORDERS (compose with the sort permutations to recover
 * original row ids).  Two-phase: call with d_out_* = NULL to get the match
 * count, then with buffers sized accordingly (state cached per call pair
 * is avoided by recomputing the cheap count pass). */
extern "C" int bg_merge_join(const int64_t* d_build_sorted, int64_t nb,
                             const int64_t* d_probe_sorted, int64_t np,
                             int64_t* out_matches, uint32_t* d_out_probe,
                             uint32_t* d_out_build) {
  REQUIRE_INIT();
  DevBuf<u64> d_counts;
  DevBuf<int64_t> d_lbs;
  DevBuf<i64> d_offs;
  DevBuf<i64> d_total;
  HIP_TRY(d_counts.alloc(np));
  HIP_TRY(d_lbs.alloc(np));
  HIP_TRY(d_offs.alloc(np));
  HIP_TRY(d_total.alloc(1));
  int blocks = grid_for(np);
  hipLaunchKernelGGL(k_merge_count, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     d_build_sorted, nb, d_probe_sorted, np, d_counts, d_lbs);
  int rc = scan_exclusive_i64(d_counts, np, d_offs, d_total);
  i64 total = 0;
  if (rc == BG_OK) {
    hipError_t e = hipMemcpy(&total, d_total, sizeof(i64),
                             hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = set_hip_err(e, "total copy");
  }
  if (rc == BG_OK && d_out_probe && d_out_build) {
    hipLaunchKernelGGL(k_merge_fill, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                       d_build_sorted, nb, np, d_offs, d_lbs, d_counts,
                       d_out_probe, d_out_build);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = set_hip_err(e, "merge fill");
  }
  if (rc == BG_OK) *out_matches = total;
  return rc;
}

// ---------------------------------------------------------------------------
// GPU Parquet decode, stage 1: Snappy page
// decompression.  Parquet compresses each page independently, so the
// parallelism unit is the PAGE: one thread decodes one page serially
// (the format is a strict byte-serial LZ77 variant), thousands of pages
// decode concurrently — throughput scales with resident pages, latency
// hidden by oversubscription.  Format: varint uncompressed length, then
// tagged elements: tag&3==0 literal (len up to 4-byte extension),
// 1 copy-1B (len 4-11, 11-bit offset), 2 copy-2B, 3 copy-4B.
// ---------------------------------------------------------------------------
// readfirstlane broadcast (SALU) — ~10x cheaper than __shfl's ds_bpermute
// for the uniform lane-0 -> wave broadcasts in byte-serial decode loops
__device__ __forceinline__ int bcast32(int v) {
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int64_t bcast64(int64_t v) {
  const int lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)((u64)v));
  const int hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((u64)v >> 32));
  return (int64_t)(((u64)(uint32_t)hi << 32) | (u64)(uint32_t)lo);
}

// Wave-cooperative decode: lane 0 walks the (strictly serial) tag stream
// and broadcasts each element; all 64 lanes execute the copy.  Overlapping
// LZ77 copies (offset < length) replicate a pattern, which parallelises as
// dst[i] = window[i % offset].  One wave per page.
__global__ void k_snappy_decompress(const bg_snappy_page* pages, int64_t npages,
                                    int64_t* out_lens /* -1 on error */) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  const int lane = lane_id();
  for (int64_t p = wave_global; p < npages; p += nwaves) {
    const uint8_t* base_s = pages[p].d_src;
    uint8_t* base_d = pages[p].d_dst;
    const int64_t src_len = pages[p].src_len;
    int64_t si = 0, di = 0;
    int64_t ulen = 0;
    int ok = 1;
    if (lane == 0) {
      int shift = 0;
      while (si < src_len) {
        const uint8_t b = base_s[si++];
        ulen |= (int64_t)(b & 0x7f) << shift;
        if (!(b & 0x80)) break;
        shift += 7;
        if (shift > 32) { ok = 0; break; }
      }
      if (ulen > pages[p].dst_cap) ok = 0;
    }
    ok = bcast32(ok);
    ulen = bcast64(ulen);
    si = bcast64(si);
    while (ok) {
      int64_t lit_len = 0, cp_len = 0, cp_off = 0, nsi = si;
      if (lane == 0 && si < src_len && di < ulen) {
        const uint8_t tag = base_s[nsi++];
        if ((tag & 3) == 0) {
          int64_t len = (tag >> 2) + 1;
          if (len > 60) {
            const int nb = (int)len - 60;
            if (nsi + nb > src_len) { ok = 0; }
            else {
              len = 0;
              for (int i = 0; i < nb; ++i)
                len |= (int64_t)base_s[nsi + i] << (8 * i);
              len += 1;
              nsi += nb;
            }
          }
          if (ok) {
            if (nsi + len > src_len || di + len > ulen) ok = 0;
            else lit_len = len;
          }
        } else {
          int64_t len = 0, off = 0;
          if ((tag & 3) == 1) {
            if (nsi >= src_len) ok = 0;
            else {
              len = ((tag >> 2) & 7) + 4;
              off = ((int64_t)(tag >> 5) << 8) | base_s[nsi];
              nsi += 1;
            }
          } else if ((tag & 3) == 2) {
            if (nsi + 2 > src_len) ok = 0;
            else {
              len = (tag >> 2) + 1;
              off = (int64_t)base_s[nsi] | ((int64_t)base_s[nsi + 1] << 8);
              nsi += 2;
            }
          } else {
            if (nsi + 4 > src_len) ok = 0;
            else {
              len = (tag >> 2) + 1;
              off = (int64_t)base_s[nsi] | ((int64_t)base_s[nsi + 1] << 8) |
                    ((int64_t)base_s[nsi + 2] << 16) |
                    ((int64_t)base_s[nsi + 3] << 24);
              nsi += 4;
            }
          }
          if (ok) {
            if (off == 0 || off > di || di + len > ulen) ok = 0;
            else { cp_len = len; cp_off = off; }
          }
        }
      }
      ok = bcast32(ok);
      if (!ok) break;
      lit_len = bcast64(lit_len);
      cp_len = bcast64(cp_len);
      cp_off = bcast64(cp_off);
      nsi = bcast64(nsi);
      if (lit_len == 0 && cp_len == 0) break;  // end of stream
      if (lit_len) {
        const uint8_t* src = base_s + nsi;
        uint8_t* dst = base_d + di;
        for (int64_t i = lane; i < lit_len; i += BG_WAVE) dst[i] = src[i];
        si = nsi + lit_len;
        di += lit_len;
      } else {
        const uint8_t* win = base_d + di - cp_off;
        uint8_t* dst = base_d + di;
        if (cp_off >= cp_len) {
          for (int64_t i = lane; i < cp_len; i += BG_WAVE) dst[i] = win[i];
        } else {
          for (int64_t i = lane; i < cp_len; i += BG_WAVE)
            dst[i] = win[i % cp_off];
        }
        si = nsi;
        di += cp_len;
      }
      if (si >= src_len || di >= ulen) break;
    }
    if (lane == 0) out_lens[p] = (ok && di == ulen) ? ulen : -1;
  }
}

// ---------------------------------------------------------------------------
// 3-pass parallel Snappy (round 2): the wave-serial decoder above peaked at
// 5.4 GB/s because ONE lane parsed tags and every element paid 4 wave
// broadcasts before 64 lanes copied ~30 bytes.  The tag stream is the only
// truly serial part, so:
//   pass 1  k_snap_parse    — one THREAD per page walks the tag stream and
//            materialises element descriptors {dst, src|off, len, kind}
//            (no copying, no broadcasts; thousands of pages in flight);
//   pass 2  k_snap_literals — every LITERAL copy is independent of all
//            other elements (source = compressed stream), so the whole
//            grid executes them wave-per-element, bandwidth-bound;
//   pass 3  k_snap_matches  — LZ77 matches replay in order per page (one
//            wave, 64-lane copies): a match window only references
//            EARLIER output bytes, and those are complete (literals from
//            pass 2, earlier matches from pass-3 order).
// Descriptor bound: every element consumes >= 2 source bytes, so
// nelems <= src_len/2 + 2.
// ---------------------------------------------------------------------------

struct SnapDesc {
  uint32_t dst;   // output byte offset
  uint32_t aux;   // literal: source offset in page; match: back offset
  uint32_t len;
  uint32_t kind;  // 0 literal, 1 match
};

// Speculative wave-parallel tag parse: every lane decodes a CANDIDATE
// element at byte si+lane (tag + extra bytes -> consumed/out_len/kind/aux,
// mostly garbage), then the wave chases the TRUE element chain through
// registers: each chase step reads the lane at the current offset via two
// u64 shuffles (no memory traffic), emits its descriptor (predicated store
// by the owning lane), and jumps to its successor.  ~24 real elements per
// 64-B window on the worst FLBA-decimal pages cost ~24 shuffle steps
// instead of 24 dependent memory round trips — the tag stream is the only
// serial part of snappy and this walks it at register speed.
__global__ void k_snap_parse(const bg_snappy_page* __restrict__ pages,
                             int64_t npages, SnapDesc* __restrict__ descs,
                             const int64_t* __restrict__ desc_base,
                             int64_t* __restrict__ counts,
                             int64_t* __restrict__ out_lens) {
  // chase staging: candidates deposited once per window, then the serial
  // chain walks LDS (~50-cy broadcast reads) instead of paired dependent
  // ds_bpermute shuffles (~600 cy/step measured)
  __shared__ uint64_t ldsq[BG_BLOCK / BG_WAVE][2 * BG_WAVE][2];
  uint64_t(*myq)[2] = ldsq[threadIdx.x / BG_WAVE];
  const int lane = lane_id();
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t p = wave_global; p < npages; p += nwaves) {
    const uint8_t* __restrict__ s = pages[p].d_src;
    const int64_t src_len = pages[p].src_len;
    SnapDesc* d = descs + desc_base[p];
    int64_t si = 0, di = 0, ulen = 0, nd = 0;
    int ok = 1, shift = 0;
    while (si < src_len) {  // uncompressed-length varint (uniform)
      const uint8_t b = s[si++];
      ulen |= (int64_t)(b & 0x7f) << shift;
      if (!(b & 0x80)) break;
      shift += 7;
      if (shift > 32) { ok = 0; break; }
    }
    if (ulen > pages[p].dst_cap) ok = 0;
    // speculative decode of the candidate element at absolute offset o
    auto spec_decode = [&](int64_t o, uint64_t* q0, uint64_t* q1,
                           int64_t rel_base) {
      *q0 = 0;
      *q1 = 0;
      if (o >= src_len) return;
      const uint8_t tag = s[o];
      const int t = tag & 3;
      int64_t next_rel = 0, out = 0;
      uint32_t aux = 0, kind = 0;
      if (t == 0) {
        int64_t len = (tag >> 2) + 1;
        int nb = 0;
        if (len > 60) {
          nb = (int)len - 60;
          if (o + 1 + nb <= src_len && nb <= 4) {
            len = 0;
            for (int i = 0; i < nb; ++i)
              len |= (int64_t)s[o + 1 + i] << (8 * i);
            len += 1;
          } else {
            len = -1;  // malformed
          }
        }
        if (len >= 0) {
          out = len;
          aux = (uint32_t)(o + 1 + nb);  // ABS literal body offset
          next_rel = rel_base + 1 + nb + len;
          kind = 0;
        }
      } else if (t == 1) {
        if (o + 1 < src_len) {
          out = ((tag >> 2) & 7) + 4;
          aux = ((uint32_t)(tag >> 5) << 8) | s[o + 1];
          next_rel = rel_base + 2;
          kind = 1;
        }
      } else if (t == 2) {
        if (o + 2 < src_len) {
          out = (tag >> 2) + 1;
          aux = (uint32_t)s[o + 1] | ((uint32_t)s[o + 2] << 8);
          next_rel = rel_base + 3;
          kind = 1;
        }
      } else {
        if (o + 4 < src_len) {
          out = (tag >> 2) + 1;
          aux = (uint32_t)s[o + 1] | ((uint32_t)s[o + 2] << 8) |
                ((uint32_t)s[o + 3] << 16) | ((uint32_t)s[o + 4] << 24);
          next_rel = rel_base + 5;
          kind = 1;
        }
      }
      if (next_rel > 0 && out >= 0 && out < ((int64_t)1 << 31) &&
          next_rel < ((int64_t)1 << 31)) {
        *q0 = ((uint64_t)(uint32_t)next_rel << 32) | (uint64_t)(uint32_t)out;
        *q1 = ((uint64_t)aux << 32) | kind;
      }
    };
    while (ok && si < src_len && di < ulen) {
      // ---- 128-B window: two candidate elements per lane ----
      uint64_t qa0, qa1, qb0, qb1;
      spec_decode(si + lane, &qa0, &qa1, lane);
      spec_decode(si + BG_WAVE + lane, &qb0, &qb1, BG_WAVE + lane);
      myq[lane][0] = qa0;
      myq[lane][1] = qa1;
      myq[BG_WAVE + lane][0] = qb0;
      myq[BG_WAVE + lane][1] = qb1;
      __builtin_amdgcn_wave_barrier();
      // prefetch the LIKELY next window while the chase runs (the chase
      // itself touches no memory beyond descriptor stores)
      {
        const int64_t pf = si + 2 * BG_WAVE + (int64_t)lane * BG_WAVE;
        if (lane < 8 && pf < src_len) {
          volatile uint8_t t_ = s[pf];
          (void)t_;
        }
      }
      // ---- chase the true chain through registers ----
      // branchless chase: errors ACCUMULATE into err and force loop exit
      // via a poisoned cur; on any error the whole page is discarded, so
      // garbage descriptors stored after the fault never surface.
      int64_t cur = 0;
      uint32_t err = 0;
      while (cur < 2 * BG_WAVE && si + cur < src_len && di < ulen) {
        const uint64_t cq0 = myq[cur][0];
        const uint64_t cq1 = myq[cur][1];
        const uint32_t next_rel = (uint32_t)(cq0 >> 32);
        const uint32_t out = (uint32_t)cq0;
        const uint32_t aux = (uint32_t)(cq1 >> 32);
        const uint32_t kind = (uint32_t)cq1 & 1;
        const uint32_t bad =
            (uint32_t)(next_rel == 0) |
            (uint32_t)(si + next_rel > src_len) |
            (uint32_t)(di + out > ulen) |
            (kind & ((uint32_t)(aux == 0) | (uint32_t)((int64_t)aux > di)));
        err |= bad;
        if (lane == 0) {
          d[nd].dst = (uint32_t)di;
          d[nd].aux = aux;
          d[nd].len = out;
          d[nd].kind = kind;
        }
        ++nd;
        di += out;
        cur = bad ? (int64_t)4 * BG_WAVE : (int64_t)next_rel;
      }
      if (err) { ok = 0; break; }
      si += cur;
    }
    if (lane == 0) {
      counts[p] = ok ? nd : 0;
      out_lens[p] = (ok && di == ulen) ? ulen : -1;
    }
  }
}

// grid.y = page (chunked to <=65535), blocks-x * waves stride elements.
// Wave-per-descriptor wasted 63 of 64 lanes on the SHORT literals that
// dominate structured pages (FLBA decimals: ~7-byte literals; 15.3 ms on
// the SF q6 parquet feed).  Each wave now takes a BATCH of 64 descriptors:
// short literals (<= 64 B) copy one-per-LANE — consecutive descriptors'
// bytes are adjacent in src and dst, so the scattered per-lane accesses
// stay within a few cache lines — and long literals replay wave-parallel
// from the ballot of survivors.
__global__ void k_snap_literals(const bg_snappy_page* __restrict__ pages,
                                int64_t page0,
                                const SnapDesc* __restrict__ descs,
                                const int64_t* __restrict__ desc_base,
                                const int64_t* __restrict__ counts) {
  const int64_t p = page0 + blockIdx.y;
  const uint8_t* src = pages[p].d_src;
  uint8_t* dst = pages[p].d_dst;
  const SnapDesc* d = descs + desc_base[p];
  const int64_t nd = counts[p];
  const int waves_per_block = blockDim.x / BG_WAVE;
  const int64_t wave = (int64_t)blockIdx.x * waves_per_block +
                       (int64_t)(threadIdx.x / BG_WAVE);
  const int64_t wstride = (int64_t)gridDim.x * waves_per_block;
  const int lane = threadIdx.x & (BG_WAVE - 1);
  if (nd <= wstride) {
    // fewer descriptors than waves (incompressible pages: a handful of
    // giant literals) — wave-per-descriptor uses every wave; batching
    // would serialise them all onto one wave (measured 295 -> 31 GB/s)
    for (int64_t e = wave; e < nd; e += wstride) {
      if (d[e].kind != 0) continue;
      const uint8_t* s = src + d[e].aux;
      uint8_t* o = dst + d[e].dst;
      const int64_t len = d[e].len;
      for (int64_t i = lane; i < len; i += BG_WAVE) o[i] = s[i];
    }
    return;
  }
  for (int64_t e0 = wave * BG_WAVE; e0 < nd; e0 += wstride * BG_WAVE) {
    const int batch = nd - e0 < BG_WAVE ? (int)(nd - e0) : BG_WAVE;
    SnapDesc my{};
    my.kind = 1;
    if (lane < batch) my = d[e0 + lane];
    if (my.kind == 0 && my.len <= BG_WAVE) {
      const uint8_t* s = src + my.aux;
      uint8_t* o = dst + my.dst;
      for (uint32_t i = 0; i < my.len; ++i) o[i] = s[i];
    }
    uint64_t longs =
        __ballot(lane < batch && my.kind == 0 && my.len > BG_WAVE);
    while (longs) {
      const int j = __builtin_ctzll(longs);
      longs &= longs - 1;
      const uint32_t aux_j = (uint32_t)__shfl((int)my.aux, j);
      const uint32_t dst_j = (uint32_t)__shfl((int)my.dst, j);
      const uint32_t len_j = (uint32_t)__shfl((int)my.len, j);
      const uint8_t* s = src + aux_j;
      uint8_t* o = dst + dst_j;
      for (uint32_t i = lane; i < len_j; i += BG_WAVE) o[i] = s[i];
    }
  }
}

// Match replay with 64-wide dependency batching: a snappy match is <= 64
// bytes, so one LANE can own one match.  Load 64 consecutive descriptors
// (coalesced); every match whose window ends BEFORE the batch's first
// output byte only reads bytes from already-completed elements, so the
// longest such prefix executes concurrently, one match per lane.  Only
// genuinely chained matches (window into the current batch — tight RLE
// runs) fall back to the one-element wave-parallel path.
__global__ void k_snap_matches(const bg_snappy_page* __restrict__ pages,
                               int64_t npages,
                               const SnapDesc* __restrict__ descs,
                               const int64_t* __restrict__ desc_base,
                               const int64_t* __restrict__ counts,
                               const uint8_t* __restrict__ skip) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  const int lane = lane_id();
  for (int64_t p = wave_global; p < npages; p += nwaves) {
    if (skip && skip[p]) continue;  // big pages replay via list ranking
    uint8_t* dst = pages[p].d_dst;
    const SnapDesc* d = descs + desc_base[p];
    const int64_t nd = counts[p];
    int64_t e = 0;
    while (e < nd) {
      const int64_t batch = nd - e < BG_WAVE ? nd - e : BG_WAVE;
      SnapDesc my{};
      if (lane < batch) my = d[e + lane];
      // consume the WHOLE batch from registers: at step j, matches whose
      // windows end before element j's output start can run one-per-lane
      // concurrently; a chained head executes wave-parallel.  No
      // descriptor reloads inside the batch.
      int j = 0;
      while (j < batch) {
        const uint32_t dst_j = (uint32_t)__shfl((int)my.dst, j);
        bool elig = lane >= j && lane < batch;
        if (elig && my.kind == 1)
          elig = ((int64_t)my.dst - (int64_t)my.aux + (int64_t)my.len <=
                  (int64_t)dst_j);
        uint64_t ball = __ballot(elig) >> j;
        int prefix = (~ball == 0) ? BG_WAVE : __builtin_ctzll(~ball);
        if (j + prefix > batch) prefix = (int)batch - j;
        if (prefix == 0) {
          const uint32_t h_off = (uint32_t)__shfl((int)my.aux, j);
          const uint32_t h_len = (uint32_t)__shfl((int)my.len, j);
          uint8_t* o = dst + dst_j;
          const uint8_t* win = o - h_off;
          if (h_off >= h_len) {
            for (uint32_t i = lane; i < h_len; i += BG_WAVE) o[i] = win[i];
          } else {
            for (uint32_t i = lane; i < h_len; i += BG_WAVE)
              o[i] = win[i % h_off];
          }
          j += 1;
        } else {
          if (lane >= j && lane < j + prefix && my.kind == 1) {
            uint8_t* o = dst + my.dst;
            const uint8_t* win = o - my.aux;
            for (uint32_t i = 0; i < my.len; ++i) o[i] = win[i];
          }
          j += prefix;
        }
        __builtin_amdgcn_wave_barrier();
      }
      e += batch;
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---------------------------------------------------------------------------
// Giant-page snappy parse (round 2): the speculative chase above is serial
// PER PAGE, so one 1-MB dict-fallback page (~300k elements) bounds the
// whole decode (~70 ms) no matter how many other pages run in parallel.
// Snappy parses SELF-SYNCHRONIZE: chains started at different offsets
// merge within a few elements.  So, for pages above a size threshold:
//   A  k_snapbig_spec    — one THREAD per 8-KB segment chases
//      speculatively from the segment start (segment 0 starts at the real
//      header end, so its chain is TRUE), recording per visited offset the
//      consumed length (membership) and prefix (count, out-bytes), plus
//      the segment's totals and exit offset.  77k segments across the
//      file run concurrently.
//   B  k_snapbig_resolve — one thread per page walks SEGMENTS (128/MB,
//      not 300k elements): if the true entry offset lands on the
//      segment's speculative chain (the common, self-synced case) the
//      whole suffix is absorbed with two subtractions; otherwise it
//      catches up element by element until it merges.  Emits per-segment
//      true entry + descriptor/output prefixes.
//   C  k_snapbig_emit    — one thread per segment re-decodes from its
//      TRUE entry and writes descriptors at the precomputed positions,
//      with the same validation as the serial parse.
// Cost: ~10 B of scratch per source byte of big pages; the per-page
// serial work drops from ~300k elements to ~128 segment steps.
// ---------------------------------------------------------------------------

#define SNAPBIG_SEG 8192   /* default; 4096 when few big pages (the
                               per-segment chase is latency-bound there
                               and shorter chases halve it; with many
                               pages the chip is throughput-bound and
                               larger segments have less overhead) */
#define SNAPBIG_THRESHOLD 98304  // pages with csz above this use A/B/C

// scalar speculative decode of the element at page-relative offset o.
// Returns false when no element can start at o (malformed/truncated).
__device__ __forceinline__ bool snap_decode_at(
    const uint8_t* __restrict__ s, int64_t src_len, int64_t o,
    int64_t* consumed, int64_t* out, uint32_t* aux, uint32_t* kind) {
  if (o >= src_len) return false;
  const uint8_t tag = s[o];
  const int t = tag & 3;
  if (t == 0) {
    int64_t len = (tag >> 2) + 1;
    int nb = 0;
    if (len > 60) {
      nb = (int)len - 60;
      if (o + 1 + nb > src_len || nb > 4) return false;
      len = 0;
      for (int i = 0; i < nb; ++i) len |= (int64_t)s[o + 1 + i] << (8 * i);
      len += 1;
    }
    *consumed = 1 + nb + len;
    *out = len;
    *aux = (uint32_t)(o + 1 + nb);
    *kind = 0;
  } else if (t == 1) {
    if (o + 1 >= src_len) return false;
    *out = ((tag >> 2) & 7) + 4;
    *aux = ((uint32_t)(tag >> 5) << 8) | s[o + 1];
    *consumed = 2;
    *kind = 1;
  } else if (t == 2) {
    if (o + 2 >= src_len) return false;
    *out = (tag >> 2) + 1;
    *aux = (uint32_t)s[o + 1] | ((uint32_t)s[o + 2] << 8);
    *consumed = 3;
    *kind = 1;
  } else {
    if (o + 4 >= src_len) return false;
    *out = (tag >> 2) + 1;
    *aux = (uint32_t)s[o + 1] | ((uint32_t)s[o + 2] << 8) |
           ((uint32_t)s[o + 3] << 16) | ((uint32_t)s[o + 4] << 24);
    *consumed = 5;
    *kind = 1;
  }
  if (*consumed <= 0 || *out < 0 || o + *consumed > src_len) return false;
  return true;
}

struct SnapBigPage {
  int64_t page_idx;  // into the bg_snappy_page array
  int64_t arr_base;  // per-byte array base (bytes)
  int64_t seg_base;  // per-seg array base
  int64_t nsegs;
  int64_t par_base;  // parent-array base (output bytes; replay phase)
  int64_t seg_sz;    // segment size this call (uniform; see SNAPBIG_SEG)
};

// phase A: speculative per-segment chase
__global__ void k_snapbig_spec(const bg_snappy_page* __restrict__ pages,
                               const SnapBigPage* __restrict__ bigs,
                               const int32_t* __restrict__ seg_page,
                               int64_t total_segs,
                               unsigned long long* dbg_ctr,
                               uint16_t* __restrict__ next16,
                               uint32_t* __restrict__ cnt_pre,
                               uint32_t* __restrict__ out_pre,
                               uint32_t* __restrict__ seg_cnt_tot,
                               uint32_t* __restrict__ seg_out_tot,
                               int64_t* __restrict__ seg_exit,
                               int64_t* __restrict__ page_hdr,
                               int64_t* __restrict__ page_ulen) {
  for (int64_t gs = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       gs < total_segs; gs += (int64_t)gridDim.x * blockDim.x) {
    const SnapBigPage& bp = bigs[seg_page[gs]];
    const int64_t k = gs - bp.seg_base;
    const bg_snappy_page& pg = pages[bp.page_idx];
    const uint8_t* s = pg.d_src;
    const int64_t src_len = pg.src_len;
    int64_t o = k * bp.seg_sz;
    if (k == 0) {
      // parse the uncompressed-length varint; segment 0 starts at the
      // TRUE element boundary
      int64_t ulen = 0, si = 0;
      int shift = 0, ok = 1;
      while (si < src_len) {
        const uint8_t b = s[si++];
        ulen |= (int64_t)(b & 0x7f) << shift;
        if (!(b & 0x80)) break;
        shift += 7;
        if (shift > 32) { ok = 0; break; }
      }
      if (ulen > pg.dst_cap) ok = 0;
      page_hdr[seg_page[gs]] = ok ? si : -1;
      page_ulen[seg_page[gs]] = ulen;
      o = si;
      if (!ok) {
        seg_exit[gs] = -1;
        seg_cnt_tot[gs] = 0;
        seg_out_tot[gs] = 0;
        continue;
      }
    }
    const int64_t seg_end =
        (k + 1) * bp.seg_sz < src_len ? (k + 1) * bp.seg_sz : src_len;
    uint32_t cnt = 0, outsum = 0;
    int64_t exitv = -1;
    while (true) {
      if (o >= seg_end) { exitv = o; break; }
      int64_t consumed, out;
      uint32_t aux, kind;
      if (!snap_decode_at(s, src_len, o, &consumed, &out, &aux, &kind)) {
        // the chase is speculative GARBAGE until it merges with the true
        // chain (which never dies on a valid page): restart one byte on.
        // Cumulative cnt/out prefixes stay consistent for the surviving
        // final fragment, which is the only one the true entry can land
        // on, so the absorb arithmetic is unaffected.
        o += 1;
        continue;
      }
      next16[bp.arr_base + o] =
          consumed > 0xFFFE ? (uint16_t)0xFFFF : (uint16_t)consumed;
      cnt_pre[bp.arr_base + o] = cnt;
      out_pre[bp.arr_base + o] = outsum;
      cnt += 1;
      outsum += (uint32_t)out;
      o += consumed;
    }
    seg_cnt_tot[gs] = cnt;
    seg_out_tot[gs] = outsum;
    seg_exit[gs] = exitv;
    if (dbg_ctr) {
      atomicAdd(&dbg_ctr[2], (unsigned long long)cnt);
      if (exitv < 0) atomicAdd(&dbg_ctr[3], 1ull);
    }
  }
}

// phase A2: parallel catch-up walks.  Phase B's serial per-page loop was
// latency-bound when few big pages exist (one THREAD per page x ~17
// dependent decodes per segment = 47 ms on a 160-page q6 feed).  But each
// segment's catch-up walk is independent under one assumption: the true
// entry into segment k is segment k-1's speculative exit (true whenever
// the true chain merged with k-1's chain — the self-synced common case).
// So walk every segment boundary in PARALLEL from that candidate entry,
// recording what the walk consumed and where it landed; phase B becomes
// an O(1)-per-segment composition that falls back to the serial walk only
// when its entry disagrees with the candidate (rare: upstream crossings).
//   w_land >= 0: landed on the segment's spec chain at this offset
//   w_land == -1: walked past the segment end (exit = w_exit)
//   w_land == -4: decode failed on the walk (malformed if entry is true)
__global__ void k_snapbig_walk(const bg_snappy_page* __restrict__ pages,
                               const SnapBigPage* __restrict__ bigs,
                               const int32_t* __restrict__ seg_page,
                               int64_t total_segs,
                               const uint16_t* __restrict__ next16,
                               const int64_t* __restrict__ seg_exit,
                               const int64_t* __restrict__ page_hdr,
                               int64_t* __restrict__ w_land,
                               int64_t* __restrict__ w_cnt,
                               int64_t* __restrict__ w_out,
                               int64_t* __restrict__ w_exit) {
  for (int64_t gs = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       gs < total_segs; gs += (int64_t)gridDim.x * blockDim.x) {
    const SnapBigPage& bp = bigs[seg_page[gs]];
    const int64_t k = gs - bp.seg_base;
    const bg_snappy_page& pg = pages[bp.page_idx];
    const uint8_t* s = pg.d_src;
    const int64_t src_len = pg.src_len;
    const int64_t e = k == 0 ? page_hdr[seg_page[gs]] : seg_exit[gs - 1];
    w_cnt[gs] = 0;
    w_out[gs] = 0;
    if (e < 0) {
      w_land[gs] = -2;  // upstream spec error; resolve goes serial
      w_exit[gs] = -1;
      continue;
    }
    const int64_t seg_end =
        (k + 1) * bp.seg_sz < src_len ? (k + 1) * bp.seg_sz : src_len;
    if (e >= seg_end) {  // candidate passes this segment entirely
      w_land[gs] = -3;
      w_exit[gs] = e;
      continue;
    }
    int64_t cur = e, cnt = 0, outsum = 0, land = -1;
    while (cur < seg_end) {
      if (next16[bp.arr_base + cur] != 0) {
        land = cur;
        break;
      }
      int64_t consumed, out;
      uint32_t aux, kind;
      if (!snap_decode_at(s, src_len, cur, &consumed, &out, &aux, &kind)) {
        land = -4;
        break;
      }
      cnt += 1;
      outsum += out;
      cur += consumed;
    }
    w_land[gs] = land;
    w_cnt[gs] = cnt;
    w_out[gs] = outsum;
    w_exit[gs] = land >= 0 ? seg_exit[gs] : cur;
  }
}

// phase B: one thread per page composes segment entries/prefixes from the
// parallel walks (serial catch-up only on candidate mismatch)
__global__ void k_snapbig_resolve(const bg_snappy_page* __restrict__ pages,
                                  const SnapBigPage* __restrict__ bigs,
                                  int64_t nbig, unsigned long long* dbg_ctr,
                                  const uint16_t* __restrict__ next16,
                                  const uint32_t* __restrict__ cnt_pre,
                                  const uint32_t* __restrict__ out_pre,
                                  const uint32_t* __restrict__ seg_cnt_tot,
                                  const uint32_t* __restrict__ seg_out_tot,
                                  const int64_t* __restrict__ seg_exit,
                                  const int64_t* __restrict__ page_hdr,
                                  const int64_t* __restrict__ page_ulen,
                                  const int64_t* __restrict__ w_land,
                                  const int64_t* __restrict__ w_cnt,
                                  const int64_t* __restrict__ w_out,
                                  const int64_t* __restrict__ w_exit,
                                  int64_t* __restrict__ seg_entry,
                                  int64_t* __restrict__ seg_nd,
                                  int64_t* __restrict__ seg_di,
                                  int64_t* __restrict__ counts,
                                  int64_t* __restrict__ out_lens) {
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nbig;
       b += (int64_t)gridDim.x * blockDim.x) {
    const SnapBigPage& bp = bigs[b];
    const bg_snappy_page& pg = pages[bp.page_idx];
    const uint8_t* s = pg.d_src;
    const int64_t src_len = pg.src_len;
    const int64_t hdr = page_hdr[b];
    const int64_t ulen = page_ulen[b];
    int err = hdr < 0;
    int64_t cur = hdr, nd = 0, di = 0;
    for (int64_t k = 0; k < bp.nsegs && !err; ++k) {
      const int64_t gs = bp.seg_base + k;
      const int64_t seg_end =
          (k + 1) * bp.seg_sz < src_len ? (k + 1) * bp.seg_sz : src_len;
      if (cur >= seg_end || di >= ulen) {
        seg_entry[gs] = -1;
        continue;
      }
      seg_entry[gs] = cur;
      seg_nd[gs] = nd;
      seg_di[gs] = di;
      const int64_t e = k == 0 ? hdr : seg_exit[gs - 1];
      const int64_t wl = w_land[gs];
      if (cur == e && wl != -2 && wl != -3) {
        // the parallel walk ran from exactly this entry: compose
        if (wl == -4) { err = 1; break; }
        nd += w_cnt[gs];
        di += w_out[gs];
        if (wl >= 0) {
          nd += (int64_t)seg_cnt_tot[gs] - cnt_pre[bp.arr_base + wl];
          di += (int64_t)seg_out_tot[gs] - out_pre[bp.arr_base + wl];
          if (seg_exit[gs] < 0) { err = 1; break; }
        }
        cur = w_exit[gs];
        if (cur < 0) { err = 1; break; }
      } else {
        // candidate mismatch: serial catch-up (rare)
        while (cur < seg_end) {
          if (next16[bp.arr_base + cur] != 0) {
            nd += (int64_t)seg_cnt_tot[gs] - cnt_pre[bp.arr_base + cur];
            di += (int64_t)seg_out_tot[gs] - out_pre[bp.arr_base + cur];
            const int64_t ex = seg_exit[gs];
            if (ex < 0) { err = 1; }
            cur = ex;
            break;
          }
          int64_t consumed, out;
          uint32_t aux, kind;
          if (!snap_decode_at(s, src_len, cur, &consumed, &out, &aux,
                              &kind)) {
            err = 1;
            break;
          }
          nd += 1;
          di += out;
          cur += consumed;
          if (dbg_ctr) atomicAdd(&dbg_ctr[1], 1ull);
        }
      }
      if (dbg_ctr) atomicAdd(&dbg_ctr[0], 1ull);
      if (di > ulen) err = 1;
    }
    // a valid stream's last element ends exactly at src_len with
    // di == ulen (snappy has no trailing bytes)
    if (!err && di != ulen) err = 1;
    counts[bp.page_idx] = err ? 0 : nd;
    out_lens[bp.page_idx] = err ? -1 : ulen;
  }
}

// phase C: one thread per live segment re-decodes its true chain and
// emits descriptors at the precomputed positions (validation included)
__global__ void k_snapbig_emit(const bg_snappy_page* __restrict__ pages,
                               const SnapBigPage* __restrict__ bigs,
                               const int32_t* __restrict__ seg_page,
                               int64_t total_segs,
                               const int64_t* __restrict__ seg_entry,
                               const int64_t* __restrict__ seg_nd,
                               const int64_t* __restrict__ seg_di,
                               const int64_t* __restrict__ page_ulen,
                               SnapDesc* __restrict__ descs,
                               const int64_t* __restrict__ desc_base,
                               int64_t* __restrict__ out_lens) {
  for (int64_t gs = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       gs < total_segs; gs += (int64_t)gridDim.x * blockDim.x) {
    if (seg_entry[gs] < 0) continue;
    const SnapBigPage& bp = bigs[seg_page[gs]];
    const int64_t k = gs - bp.seg_base;
    const bg_snappy_page& pg = pages[bp.page_idx];
    const uint8_t* s = pg.d_src;
    const int64_t src_len = pg.src_len;
    const int64_t ulen = page_ulen[seg_page[gs]];
    const int64_t seg_end =
        (k + 1) * bp.seg_sz < src_len ? (k + 1) * bp.seg_sz : src_len;
    SnapDesc* d = descs + desc_base[bp.page_idx];
    int64_t cur = seg_entry[gs];
    int64_t nd = seg_nd[gs], di = seg_di[gs];
    while (cur < seg_end && di < ulen) {
      int64_t consumed, out;
      uint32_t aux, kind;
      if (!snap_decode_at(s, src_len, cur, &consumed, &out, &aux, &kind)) {
        atomicExch((unsigned long long*)&out_lens[bp.page_idx],
                   (unsigned long long)(-1LL));
        return;
      }
      if (di + out > ulen ||
          (kind == 1 && (aux == 0 || (int64_t)aux > di))) {
        atomicExch((unsigned long long*)&out_lens[bp.page_idx],
                   (unsigned long long)(-1LL));
        return;
      }
      d[nd].dst = (uint32_t)di;
      d[nd].aux = aux;
      d[nd].len = (uint32_t)out;
      d[nd].kind = kind;
      ++nd;
      di += out;
      cur += consumed;
    }
  }
}

// ---------------------------------------------------------------------------
// Giant-page match REPLAY by list ranking (round 2, final): the in-order
// wave replay (k_snap_matches) is serial per page, so one 1-MB page with
// ~150k matches bounds the decode no matter how many pages run.  But the
// copy structure is a FOREST: every output byte of a match has exactly ONE
// parent byte — the window byte it copies, (dst-aux) + ((b-dst) mod aux)
// (the mod makes overlapping/RLE matches periodic fills of the pre-match
// window, exactly the serial semantics) — and parents always point
// strictly backward, with literal bytes as roots.  So:
//   par_init     P[b] = b                     (literal bytes stay roots)
//   par_scatter  match descs write their bytes' parents     (parallel)
//   par_double   P[b] = P^4[b] until fixpoint (jump-4 pointer doubling:
//                ceil(log4 depth) rounds; measured chain depths 200-1000
//                => 5-6 rounds; races only jump FURTHER toward the root,
//                so the passes are correct without any synchronisation)
//   par_fill     dst[b] = dst[P[b]]           (after literals land; every
//                root is a literal byte, so one unordered gather)
// The doubling/fill loops are XCD-swizzled: page -> XCD by index so each
// page's parent array (4 B/byte; 4 MB for a 1-MB page) lives in ONE
// XCD's L2 instead of thrashing all eight.
// ---------------------------------------------------------------------------

__global__ void k_snap_par_init(const SnapBigPage* __restrict__ bigs,
                                int64_t nbig,
                                const int64_t* __restrict__ lens,
                                uint32_t* __restrict__ P) {
  const int xcd = blockIdx.x & 7;
  const int slot = blockIdx.x >> 3;
  const int64_t nslot = gridDim.x >> 3;
  for (int64_t bi = xcd; bi < nbig; bi += 8) {
    const SnapBigPage& bp = bigs[bi];
    const int64_t ulen = lens[bp.page_idx];
    if (ulen <= 0) continue;
    uint32_t* p = P + bp.par_base;
    for (int64_t b = slot * blockDim.x + threadIdx.x; b < ulen;
         b += nslot * blockDim.x)
      p[b] = (uint32_t)b;
  }
}

__global__ void k_snap_par_scatter(const SnapDesc* __restrict__ descs,
                                   const int64_t* __restrict__ desc_base,
                                   const int64_t* __restrict__ counts,
                                   const SnapBigPage* __restrict__ bigs,
                                   int64_t big0,
                                   const int64_t* __restrict__ lens,
                                   uint32_t* __restrict__ P) {
  const SnapBigPage& bp = bigs[big0 + blockIdx.y];
  if (lens[bp.page_idx] <= 0) return;
  const SnapDesc* d = descs + desc_base[bp.page_idx];
  const int64_t nd = counts[bp.page_idx];
  uint32_t* p = P + bp.par_base;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nd;
       e += (int64_t)gridDim.x * blockDim.x) {
    if (d[e].kind != 1) continue;
    const uint32_t dst = d[e].dst, aux = d[e].aux, len = d[e].len;
    const uint32_t base = dst - aux;  // aux <= dst validated at emit
    if (aux >= len) {
      for (uint32_t i = 0; i < len; ++i) p[dst + i] = base + i;
    } else {
      for (uint32_t i = 0; i < len; ++i) p[dst + i] = base + (i % aux);
    }
  }
}

__global__ void k_snap_par_double(const SnapBigPage* __restrict__ bigs,
                                  int64_t nbig,
                                  const int64_t* __restrict__ lens,
                                  uint32_t* __restrict__ P,
                                  int* __restrict__ changed) {
  const int xcd = blockIdx.x & 7;
  const int slot = blockIdx.x >> 3;
  const int64_t nslot = gridDim.x >> 3;
  int any = 0;
  for (int64_t bi = xcd; bi < nbig; bi += 8) {
    const SnapBigPage& bp = bigs[bi];
    const int64_t ulen = lens[bp.page_idx];
    if (ulen <= 0) continue;
    uint32_t* p = P + bp.par_base;
    for (int64_t b = slot * blockDim.x + threadIdx.x; b < ulen;
         b += nslot * blockDim.x) {
      const uint32_t r0 = p[b];
      const uint32_t r1 = p[r0];
      if (r1 == r0) continue;  // already at root
      // jump-4; jump-8 measured WORSE (flba7 double 5.0 -> 5.8 ms, runs
      // 17.4 -> 15.7 GB/s): the longer dependent-load chain costs more
      // than the saved write passes
      const uint32_t r2 = p[r1];
      const uint32_t r3 = p[r2];
      p[b] = p[r3];
      any = 1;
    }
  }
  if (any) *changed = 1;
}

__global__ void k_snap_par_fill(const bg_snappy_page* __restrict__ pages,
                                const SnapBigPage* __restrict__ bigs,
                                int64_t nbig,
                                const int64_t* __restrict__ lens,
                                const uint32_t* __restrict__ P) {
  const int xcd = blockIdx.x & 7;
  const int slot = blockIdx.x >> 3;
  const int64_t nslot = gridDim.x >> 3;
  for (int64_t bi = xcd; bi < nbig; bi += 8) {
    const SnapBigPage& bp = bigs[bi];
    const int64_t ulen = lens[bp.page_idx];
    if (ulen <= 0) continue;
    const uint32_t* p = P + bp.par_base;
    uint8_t* out = pages[bp.page_idx].d_dst;
    for (int64_t b = slot * blockDim.x + threadIdx.x; b < ulen;
         b += nslot * blockDim.x) {
      const uint32_t r = p[b];
      if ((int64_t)r != b) out[b] = out[r];
    }
  }
}

// ---- bg_snappy_decompress host side: route -> parse -> literals ->
// replay -> matches, one static function per phase ----

// device arrays every phase of one call shares
struct SnapDev {
  DevBuf<bg_snappy_page> pages;
  DevBuf<int64_t> lens, base, counts;
  DevBuf<SnapDesc> descs;
};

// the host-side routing decision of one call
struct SnapRoute {
  std::vector<SnapBigPage> bigs;       // pages for the segmented parse
  std::vector<int32_t> seg_page;       // segment -> index into bigs
  int64_t segsz = 0;                   // segment size this call
  int64_t arr_total = 0;               // per-byte array elements over bigs
  int64_t seg_total = 0;               // segments over bigs
  std::vector<SnapBigPage> par_pages;  // pages replayed by list ranking
};

// BG_SNAPPY_DEBUG wall clock in ms (drains the device); 0 when disabled
static double snap_tick(bool dbg) {
  if (!dbg) return 0.0;
  (void)hipDeviceSynchronize();
  return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
             .count() / 1e6;
}

static bool snap_is_big(const bg_snappy_page& pg) {
  if (pg.src_len <= SNAPBIG_THRESHOLD) return false;
  if (pg.dst_cap > 0 && (double)pg.src_len > 0.85 * (double)pg.dst_cap)
    return false;
  return true;
}

// Pure host step (no HIP call): which pages take the segmented parse and
// which are replayed by list ranking.
static SnapRoute snap_route(const bg_snappy_page* hp, int64_t npages) {
  SnapRoute r;
  // giant pages (dict-fallback ~1 MB pages) go through the segmented
  // self-synchronizing parse; the wave chase handles the rest.  The
  // chase kernel still runs over ALL pages but exits immediately for big
  // ones (counts/lens are overwritten by phase B/C afterwards) — to keep
  // it simple we simply run the chase on the small pages only by
  // swapping big pages out of its view via a filtered page list.
  // route to the segmented path: big AND element-dense.  Near-
  // incompressible pages are literal-dominated (few elements) and the
  // wave chase handles them at full rate.
  int64_t nbig_est = 0;
  for (int64_t p = 0; p < npages; ++p)
    if (snap_is_big(hp[p])) ++nbig_est;
  r.segsz = nbig_est <= 768 ? SNAPBIG_SEG / 2 : SNAPBIG_SEG;
  for (int64_t p = 0; p < npages; ++p) {
    if (!snap_is_big(hp[p])) continue;
    SnapBigPage bp;
    bp.page_idx = p;
    bp.arr_base = r.arr_total;
    bp.seg_base = r.seg_total;
    bp.nsegs = (hp[p].src_len + r.segsz - 1) / r.segsz;
    bp.seg_sz = r.segsz;
    bp.par_base = 0;
    r.arr_total += hp[p].src_len;
    for (int64_t k = 0; k < bp.nsegs; ++k)
      r.seg_page.push_back((int32_t)r.bigs.size());
    r.seg_total += bp.nsegs;
    r.bigs.push_back(bp);
  }
  // List-ranking replay routing — INDEPENDENT of the segmented-parse
  // routing above: replay cost is set by matches x chain depth, not by
  // compressed size, so it also covers highly-expanding pages whose
  // compressed bytes are small (1-MB RLE "runs" pages: 50 KB compressed,
  // 16k matches chained 1000 deep — 1.35 GB/s serial).  Eligible: output
  // large enough that the serial in-order replay is the bound, not
  // near-incompressible (replay there is trivial), output size declared
  // (parent arrays are 4 B per output byte).  With MANY such pages the
  // serial per-page replay already fills the chip (one wave per page)
  // and the doubling passes' extra traffic loses — measured crossover
  // ~700 1-MB pages (160: 6.2 ms vs 23 ms serial; 2000: 55 vs 25 ms).
  // Two eligibility classes (both need a declared output size <= 4 GB):
  //   A — heavy-RLE pages (csz < 0.15 x usz): their match chains are deep
  //       (offset-1 runs), so the serial replay is a per-page ~100 ms
  //       latency wall no matter how many pages run concurrently (1-MB
  //       runs pages: 7.3 us/descriptor).  ALWAYS list-rank, any count.
  //   B — moderate-expansion pages: serial replay is throughput-bound and
  //       page-parallelism covers it once enough pages exist — measured
  //       crossover ~700 1-MB pages (160: 6.2 ms parents vs 23 ms serial;
  //       2000: 55 vs 25 ms).  List-rank only when the count is low.
  // The combined set is processed in chunks of <= 4 GB of parent arrays
  // to bound replay memory.
  bool caps_ok = true;
  int64_t class_b = 0;
  for (int64_t p = 0; p < npages; ++p) {
    const int64_t cap = hp[p].dst_cap;
    if (cap <= (int64_t)131072) continue;
    const double ratio = (double)hp[p].src_len / (double)cap;
    if (ratio > 0.85) continue;
    if (cap > (int64_t)UINT32_MAX) {
      caps_ok = false;
      break;
    }
    SnapBigPage pp{};
    pp.page_idx = p;
    pp.par_base = ratio < 0.15 ? -1 : 0;  // -1 marks class A for the cut
    r.par_pages.push_back(pp);
    if (pp.par_base == 0) ++class_b;
  }
  if (!caps_ok) {
    r.par_pages.clear();
  } else if (class_b > 768) {
    // keep only class A
    std::vector<SnapBigPage> keep;
    for (auto& pp : r.par_pages)
      if (pp.par_base < 0) keep.push_back(pp);
    r.par_pages.swap(keep);
  }
  return r;
}

// Wave-chase parse of every page the segmented parse does not take:
// directly over the full page list when there is no big page, otherwise on
// a compacted list whose counts/lens are scattered back to the full arrays.
static int snap_parse_small(const SnapDev& d, const bg_snappy_page* hp,
                            const std::vector<int64_t>& base, int64_t npages,
                            bool any_big) {
  const int wpb1 = BG_BLOCK / BG_WAVE;  // parse waves per block
  if (!any_big) {
    int blocks1 = grid_for(npages, wpb1);
    hipLaunchKernelGGL(k_snap_parse, dim3(blocks1), dim3(BG_BLOCK), 0, 0,
                       d.pages.get(), npages, d.descs.get(), d.base.get(),
                       d.counts.get(), d.lens.get());
    HIP_TRY(hipGetLastError());
    return BG_OK;
  }
  // small pages via the chase (on a compacted page list mapped back)
  std::vector<bg_snappy_page> smalls;
  std::vector<int64_t> small_map, small_base;
  for (int64_t p = 0; p < npages; ++p) {
    if (snap_is_big(hp[p])) continue;
    smalls.push_back(hp[p]);
    small_map.push_back(p);
    small_base.push_back(base[p]);
  }
  if (smalls.empty()) return BG_OK;
  const int64_t ns = (int64_t)smalls.size();
  DevBuf<bg_snappy_page> d_small;
  DevBuf<int64_t> d_small_base, d_small_counts, d_small_lens;
  HIP_TRY(d_small.alloc(ns));
  HIP_TRY(d_small_base.alloc(ns));
  HIP_TRY(d_small_counts.alloc(ns));
  HIP_TRY(d_small_lens.alloc(ns));
  HIP_TRY(hipMemcpy(d_small, smalls.data(), sizeof(bg_snappy_page) * ns,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_small_base, small_base.data(), sizeof(int64_t) * ns,
                    hipMemcpyHostToDevice));
  int sb = grid_for(ns, wpb1);
  hipLaunchKernelGGL(k_snap_parse, dim3(sb), dim3(BG_BLOCK), 0, 0,
                     d_small.get(), ns, d.descs.get(), d_small_base.get(),
                     d_small_counts.get(), d_small_lens.get());
  HIP_TRY(hipGetLastError());
  // scatter counts/lens back to the full arrays
  std::vector<int64_t> tmpc(ns), tmpl(ns);
  HIP_TRY(hipMemcpy(tmpc.data(), d_small_counts, sizeof(int64_t) * ns,
                    hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tmpl.data(), d_small_lens, sizeof(int64_t) * ns,
                    hipMemcpyDeviceToHost));
  std::vector<int64_t> full_c(npages, 0), full_l(npages, 0);
  for (int64_t i = 0; i < ns; ++i) {
    full_c[small_map[i]] = tmpc[i];
    full_l[small_map[i]] = tmpl[i];
  }
  HIP_TRY(hipMemcpy(d.counts, full_c.data(), sizeof(int64_t) * npages,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.lens, full_l.data(), sizeof(int64_t) * npages,
                    hipMemcpyHostToDevice));
  return BG_OK;
}

// Segmented self-synchronizing parse of the big pages:
// A (spec) -> walk -> B (resolve) -> C (emit)
static int snap_parse_segmented(const SnapDev& d, const SnapRoute& r,
                                bool dbg) {
  const int64_t nbig = (int64_t)r.bigs.size();
  const int64_t seg_total = r.seg_total, arr_total = r.arr_total;
  DevBuf<SnapBigPage> d_bigs;
  DevBuf<int32_t> d_seg_page;
  DevBuf<uint16_t> d_next16;
  DevBuf<uint32_t> d_cnt_pre, d_out_pre, d_seg_ct, d_seg_ot;
  DevBuf<int64_t> d_seg_exit, d_seg_entry, d_seg_nd, d_seg_di;
  DevBuf<int64_t> d_page_hdr, d_page_ulen;
  HIP_TRY(d_bigs.alloc(nbig));
  HIP_TRY(d_seg_page.alloc(seg_total));
  HIP_TRY(d_next16.alloc(arr_total));
  HIP_TRY(d_cnt_pre.alloc(arr_total));
  HIP_TRY(d_out_pre.alloc(arr_total));
  HIP_TRY(d_seg_ct.alloc(seg_total));
  HIP_TRY(d_seg_ot.alloc(seg_total));
  HIP_TRY(d_seg_exit.alloc(seg_total));
  HIP_TRY(d_seg_entry.alloc(seg_total));
  HIP_TRY(d_seg_nd.alloc(seg_total));
  HIP_TRY(d_seg_di.alloc(seg_total));
  HIP_TRY(d_page_hdr.alloc(nbig));
  HIP_TRY(d_page_ulen.alloc(nbig));
  HIP_TRY(hipMemcpy(d_bigs, r.bigs.data(), sizeof(SnapBigPage) * nbig,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_seg_page, r.seg_page.data(),
                    sizeof(int32_t) * seg_total, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_next16, 0, sizeof(uint16_t) * arr_total));
  int ab = grid_for(seg_total);
  DevBuf<unsigned long long> d_dbg;  // 4 debug counters; null unless dbg
  if (dbg) {
    HIP_TRY(d_dbg.alloc(4));
    HIP_TRY(hipMemset(d_dbg, 0, 32));
  }

  double tb0 = snap_tick(dbg);
  hipLaunchKernelGGL(k_snapbig_spec, dim3(ab), dim3(BG_BLOCK), 0, 0,
                     d.pages.get(), d_bigs.get(), d_seg_page.get(), seg_total,
                     d_dbg.get(), d_next16.get(), d_cnt_pre.get(),
                     d_out_pre.get(), d_seg_ct.get(), d_seg_ot.get(),
                     d_seg_exit.get(), d_page_hdr.get(), d_page_ulen.get());
  HIP_TRY(hipGetLastError());
  double tb1 = snap_tick(dbg);
  DevBuf<int64_t> d_w_land, d_w_cnt, d_w_out, d_w_exit;
  HIP_TRY(d_w_land.alloc(seg_total));
  HIP_TRY(d_w_cnt.alloc(seg_total));
  HIP_TRY(d_w_out.alloc(seg_total));
  HIP_TRY(d_w_exit.alloc(seg_total));
  hipLaunchKernelGGL(k_snapbig_walk, dim3(ab), dim3(BG_BLOCK), 0, 0,
                     d.pages.get(), d_bigs.get(), d_seg_page.get(), seg_total,
                     d_next16.get(), d_seg_exit.get(), d_page_hdr.get(),
                     d_w_land.get(), d_w_cnt.get(), d_w_out.get(),
                     d_w_exit.get());
  HIP_TRY(hipGetLastError());
  double tb1b = snap_tick(dbg);
  int bb = grid_for(nbig);
  hipLaunchKernelGGL(k_snapbig_resolve, dim3(bb), dim3(BG_BLOCK), 0, 0,
                     d.pages.get(), d_bigs.get(), nbig, d_dbg.get(),
                     d_next16.get(), d_cnt_pre.get(), d_out_pre.get(),
                     d_seg_ct.get(), d_seg_ot.get(), d_seg_exit.get(),
                     d_page_hdr.get(), d_page_ulen.get(), d_w_land.get(),
                     d_w_cnt.get(), d_w_out.get(), d_w_exit.get(),
                     d_seg_entry.get(), d_seg_nd.get(), d_seg_di.get(),
                     d.counts.get(), d.lens.get());
  HIP_TRY(hipGetLastError());
  // the walk outputs are dead after resolve: back to the pool before emit
  d_w_land.reset();
  d_w_cnt.reset();
  d_w_out.reset();
  d_w_exit.reset();
  double tb2 = snap_tick(dbg);
  hipLaunchKernelGGL(k_snapbig_emit, dim3(ab), dim3(BG_BLOCK), 0, 0,
                     d.pages.get(), d_bigs.get(), d_seg_page.get(), seg_total,
                     d_seg_entry.get(), d_seg_nd.get(), d_seg_di.get(),
                     d_page_ulen.get(), d.descs.get(), d.base.get(),
                     d.lens.get());
  HIP_TRY(hipGetLastError());
  if (dbg) {
    double tb3 = snap_tick(dbg);
    unsigned long long hc[4] = {0, 0, 0, 0};
    (void)hipMemcpy(hc, d_dbg, 32, hipMemcpyDeviceToHost);
    fprintf(stderr,
            "[bg_snappy]   big: nseg=%lld spec=%.3fms walk=%.3fms "
            "resolve=%.3fms emit=%.3fms seg_steps=%llu catchup=%llu "
            "spec_elems=%llu spec_died=%llu\n",
            (long long)seg_total, tb1 - tb0, tb1b - tb1, tb2 - tb1b,
            tb3 - tb2, hc[0], hc[1], hc[2], hc[3]);
  }
  return BG_OK;
}

// List-ranking replay of par_pages (parents are built here, after the
// literal roots have landed), in chunks of <= 4 GB of parent arrays:
// init, scatter, up to 20 doubling rounds, fill.
static int snap_replay_listrank(const SnapDev& d, const bg_snappy_page* hp,
                                const std::vector<SnapBigPage>& par_pages,
                                bool dbg, int* par_rounds) {
  DevBuf<int> d_changed;
  HIP_TRY(d_changed.alloc(1));
  const int64_t CHUNK_ELEMS = ((int64_t)4 << 30) / sizeof(uint32_t);
  const int pb = 1024;  // multiple of 8: page->XCD swizzle
  double tp_init = 0, tp_scat = 0, tp_dbl = 0, tp_fill = 0;
  size_t ci = 0;
  while (ci < par_pages.size()) {
    std::vector<SnapBigPage> chunk;
    int64_t elems = 0;
    while (ci < par_pages.size()) {
      const int64_t cap = hp[par_pages[ci].page_idx].dst_cap;
      if (!chunk.empty() && elems + cap > CHUNK_ELEMS) break;
      SnapBigPage pp = par_pages[ci];
      pp.par_base = elems;
      elems += cap;
      chunk.push_back(pp);
      ++ci;
    }
    const int64_t npar = (int64_t)chunk.size();
    DevBuf<SnapBigPage> d_parp;  // per chunk: released at the end of each turn
    DevBuf<uint32_t> d_par;
    HIP_TRY(d_parp.alloc(npar));
    // (a fallback to the serial replay when this fails goes here)
    HIP_TRY(d_par.alloc(elems));
    HIP_TRY(hipMemcpy(d_parp, chunk.data(), sizeof(SnapBigPage) * npar,
                      hipMemcpyHostToDevice));
    double tp0 = snap_tick(dbg);
    hipLaunchKernelGGL(k_snap_par_init, dim3(pb), dim3(BG_BLOCK), 0, 0,
                       d_parp.get(), npar, d.lens.get(), d_par.get());
    HIP_TRY(hipGetLastError());
    double tp1 = snap_tick(dbg);
    for (int64_t b0 = 0; b0 < npar; b0 += 65535) {
      uint32_t ny = (uint32_t)bg_imin64(npar - b0, 65535);
      hipLaunchKernelGGL(k_snap_par_scatter, dim3(64, ny), dim3(BG_BLOCK), 0,
                         0, d.descs.get(), d.base.get(), d.counts.get(),
                         d_parp.get(), b0, d.lens.get(), d_par.get());
      HIP_TRY(hipGetLastError());
    }
    double tp2 = snap_tick(dbg);
    // jump-4 doubling: parents strictly decrease (validated at parse),
    // so convergence is guaranteed; x4 path compression per round
    for (int round = 0; round < 20; ++round) {
      HIP_TRY(hipMemset(d_changed, 0, sizeof(int)));
      hipLaunchKernelGGL(k_snap_par_double, dim3(pb), dim3(BG_BLOCK), 0, 0,
                         d_parp.get(), npar, d.lens.get(), d_par.get(),
                         d_changed.get());
      HIP_TRY(hipGetLastError());
      int h_changed = 0;
      HIP_TRY(hipMemcpy(&h_changed, d_changed, sizeof(int),
                        hipMemcpyDeviceToHost));
      ++*par_rounds;
      if (!h_changed) break;
    }
    double tp3 = snap_tick(dbg);
    hipLaunchKernelGGL(k_snap_par_fill, dim3(pb), dim3(BG_BLOCK), 0, 0,
                       d.pages.get(), d_parp.get(), npar, d.lens.get(),
                       d_par.get());
    HIP_TRY(hipGetLastError());
    d_parp.reset();
    d_par.reset();
    if (dbg) {
      double tp4 = snap_tick(dbg);
      tp_init += tp1 - tp0;
      tp_scat += tp2 - tp1;
      tp_dbl += tp3 - tp2;
      tp_fill += tp4 - tp3;
    }
  }
  if (dbg)
    fprintf(stderr,
            "[bg_snappy]   par: npar=%lld init=%.3fms scatter=%.3fms "
            "double=%.3fms fill=%.3fms\n",
            (long long)par_pages.size(), tp_init, tp_scat, tp_dbl, tp_fill);
  return BG_OK;
}

/* Decompress npages independent Snappy blocks.  pages: HOST array copied
 * internally; each entry's src/dst are DEVICE pointers.  out_lens (host,
 * npages): decompressed length or -1 on malformed input. */
extern "C" int bg_snappy_decompress(const bg_snappy_page* h_pages,
                                    int64_t npages, int64_t* h_out_lens) {
  REQUIRE_INIT();
  if (npages <= 0) return BG_OK;
  const bg_snappy_page* hp = h_pages;
  std::vector<int64_t> base(npages + 1);
  base[0] = 0;
  for (int64_t p = 0; p < npages; ++p)
    base[p + 1] = base[p] + hp[p].src_len / 2 + 2;
  SnapDev d;
  HIP_TRY(d.pages.alloc(npages));
  HIP_TRY(d.lens.alloc(npages));
  HIP_TRY(d.base.alloc(npages + 1));
  HIP_TRY(d.counts.alloc(npages));
  HIP_TRY(d.descs.alloc(base[npages]));
  HIP_TRY(hipMemcpy(d.pages, h_pages, sizeof(bg_snappy_page) * npages,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.base, base.data(), sizeof(int64_t) * (npages + 1),
                    hipMemcpyHostToDevice));
  const bool dbg = getenv("BG_SNAPPY_DEBUG") != nullptr;
  const SnapRoute route = snap_route(hp, npages);

  // parse: the wave chase for small pages, the segmented parse for big ones
  double t0 = snap_tick(dbg);
  const bool any_big = !route.bigs.empty();
  if (int rc = snap_parse_small(d, hp, base, npages, any_big)) return rc;
  if (any_big)
    if (int rc = snap_parse_segmented(d, route, dbg)) return rc;
  double t1 = snap_tick(dbg);

  // literals — pass 2: chunk grid.y at 65535 pages
  const int waves_per_block = BG_BLOCK / BG_WAVE;
  // enough x-blocks to spread big pages' literal lists over the chip
  int xb = (int)bg_imin64(
      (16384 + npages - 1) / (npages > 0 ? npages : 1) + 1, 1024);
  for (int64_t p0 = 0; p0 < npages; p0 += 65535) {
    uint32_t ny = (uint32_t)bg_imin64(npages - p0, 65535);
    hipLaunchKernelGGL(k_snap_literals, dim3((uint32_t)xb, ny),
                       dim3(BG_BLOCK), 0, 0, d.pages.get(), p0,
                       d.descs.get(), d.base.get(), d.counts.get());
    HIP_TRY(hipGetLastError());
  }
  double t2 = snap_tick(dbg);

  // replay: list ranking for the routed pages; k_snap_matches skips them
  double t_par = 0;
  int par_rounds = 0;
  DevBuf<uint8_t> d_isbig;  // stays null when no page is list-ranked
  if (!route.par_pages.empty()) {
    std::vector<uint8_t> isbig(npages, 0);
    for (auto& pp : route.par_pages) isbig[pp.page_idx] = 1;
    HIP_TRY(d_isbig.alloc(npages));
    HIP_TRY(hipMemcpy(d_isbig, isbig.data(), npages, hipMemcpyHostToDevice));
    if (int rc = snap_replay_listrank(d, hp, route.par_pages, dbg,
                                      &par_rounds))
      return rc;
    if (dbg) t_par = snap_tick(dbg) - t2;
  }

  // matches: the serial in-order replay of every other page
  double t2b = snap_tick(dbg);
  int blocks3 = grid_for(npages, waves_per_block);
  hipLaunchKernelGGL(k_snap_matches, dim3(blocks3), dim3(BG_BLOCK), 0, 0,
                     d.pages.get(), npages, d.descs.get(), d.base.get(),
                     d.counts.get(), d_isbig.get());
  HIP_TRY(hipGetLastError());
  if (dbg)
    fprintf(stderr,
            "[bg_snappy] npages=%lld parse=%.3fms literals=%.3fms "
            "par=%.3fms(rounds=%d) matches=%.3fms\n",
            (long long)npages, t1 - t0, t2 - t1, t_par, par_rounds + 1,
            snap_tick(dbg) - t2b);
  d_isbig.reset();
  HIP_TRY(hipMemcpy(h_out_lens, d.lens, sizeof(int64_t) * npages,
                    hipMemcpyDeviceToHost));
  return BG_OK;
}

// ULEB128 varint shared by every Parquet page walker below: reads at most 10
// bytes (shift <= 63) from [d, end).  A varint cut off by `end`, or one
// still continuing after 10 bytes, is malformed: returns false.
__device__ __forceinline__ bool bg_uvarint(const uint8_t*& d,
                                           const uint8_t* end, u64* out_v) {
  u64 v = 0;
  for (int sh = 0; sh <= 63 && d < end; sh += 7) {
    const uint8_t b = *d++;
    v |= (u64)(b & 0x7f) << sh;
    if (!(b & 0x80)) { *out_v = v; return true; }
  }
  return false;
}

// ---------------------------------------------------------------------------
// Parquet data-page extraction (PLAIN values, no nulls):
// optional columns prefix the page with [u32 len][RLE/bit-packed def
// levels]; thread 0 validates every def level == 1 (a null anywhere =>
// error: null decode is a later row), then the block copies the PLAIN
// value bytes to the column buffer; FLBA(16) decimals (parquet big-endian)
// are byte-reversed to Arrow little-endian in flight.
// ---------------------------------------------------------------------------
__device__ void k_page_extract_body(const uint8_t* page, int64_t page_len,
                                    uint8_t* out, int64_t nvals,
                                    int64_t src_esz, int has_def,
                                    int flba_reverse, const uint32_t* vidx,
                                    const int64_t* n_present, int* err) {
  __shared__ int64_t s_voff;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t voff = 0;
    int ok = 1;
    if (has_def == 2) {
      // nullable: levels already decoded by bg_def_levels_batch — just
      // skip past them and bound the packed value section
      if (page_len < 4) ok = 0;
      else {
        const uint32_t dlen = (uint32_t)page[0] | ((uint32_t)page[1] << 8) |
                              ((uint32_t)page[2] << 16) |
                              ((uint32_t)page[3] << 24);
        voff = 4 + (int64_t)dlen;
        if (voff + (*n_present) * src_esz > page_len) ok = 0;
      }
      if (!ok) atomicExch(err, 2);
      s_voff = ok ? voff : -1;
    } else if (has_def) {
      uint32_t dlen = 0;
      if (page_len < 4) ok = 0;
      else {
        dlen = (uint32_t)page[0] | ((uint32_t)page[1] << 8) |
               ((uint32_t)page[2] << 16) | ((uint32_t)page[3] << 24);
        if ((int64_t)dlen > page_len - 4) { ok = 0; dlen = 0; }
      }
      // walk the RLE/bit-packed hybrid (bit width 1): every level must be 1
      const uint8_t* d = page + 4;
      const uint8_t* dend = d + dlen;
      int64_t seen = 0;
      while (d < dend && seen < nvals && ok) {
        u64 header = 0;
        if (!bg_uvarint(d, dend, &header)) { ok = 0; break; }
        if (header & 1) {  // bit-packed group: (count/8)<<1|1, 1 byte per 8
          const int64_t groups = (int64_t)(header >> 1);
          for (int64_t g = 0; g < groups && ok; ++g) {
            if (d >= dend) { ok = 0; break; }
            const uint8_t byte = *d++;
            const int64_t take = nvals - seen >= 8 ? 8 : nvals - seen;
            for (int64_t t = 0; t < take; ++t)
              if (!((byte >> t) & 1)) ok = 0;
            seen += take;
          }
        } else {  // RLE run: count<<1, value in 1 byte (bit width <= 8)
          const int64_t run = (int64_t)(header >> 1);
          if (d >= dend) { ok = 0; break; }
          const uint8_t val = *d++;
          if (val != 1) ok = 0;
          seen += run < nvals - seen ? run : nvals - seen;
        }
      }
      if (seen < nvals) ok = 0;
      voff = 4 + dlen;
      if (voff + nvals * src_esz > page_len) ok = 0;  // geometry bound
      if (!ok) atomicExch(err, 2);  // malformed / unexpected nulls
      s_voff = ok ? voff : -1;
    } else {
      if (voff + nvals * src_esz > page_len) ok = 0;  // geometry bound
      if (!ok) atomicExch(err, 2);
      s_voff = ok ? voff : -1;
    }
  }
  __syncthreads();
  const int64_t voff = s_voff;
  if (voff < 0) return;
  if (has_def == 2) {
    // scatter the packed value stream to its slots (NULL slots untouched)
    for (int64_t v = threadIdx.x; v < nvals; v += blockDim.x) {
      const uint32_t ix = vidx[v];
      if (ix == 0xffffffffu) continue;
      const uint8_t* src = page + voff + (int64_t)ix * src_esz;
      uint8_t* dst = out + v * (flba_reverse ? 16 : src_esz);
      if (!flba_reverse) {
        for (int64_t b = 0; b < src_esz; ++b) dst[b] = src[b];
      } else {
        const uint8_t sign = (src[0] & 0x80) ? 0xff : 0x00;
        for (int64_t b = 0; b < 16; ++b)
          dst[b] = (b < src_esz) ? src[src_esz - 1 - b] : sign;
      }
    }
    return;
  }
  if (!flba_reverse) {
    const int64_t nbytes = nvals * src_esz;
    for (int64_t i = threadIdx.x; i < nbytes; i += blockDim.x)
      out[i] = page[voff + i];
  } else {
    // FLBA(src_esz) big-endian two's complement -> 16-byte LE decimal128
    // with sign extension (parquet stores decimals at the minimal width
    // for the precision, e.g. 7 bytes for Decimal(15,2))
    for (int64_t v = threadIdx.x; v < nvals; v += blockDim.x) {
      const uint8_t* src = page + voff + v * src_esz;
      uint8_t* dst = out + v * 16;
      const uint8_t sign = (src[0] & 0x80) ? 0xff : 0x00;
      for (int64_t b = 0; b < 16; ++b)
        dst[b] = (b < src_esz) ? src[src_esz - 1 - b] : sign;
    }
  }
}

__global__ void k_page_extract(const uint8_t* page, int64_t page_len,
                               uint8_t* out, int64_t nvals, int64_t src_esz,
                               int has_def, int flba_reverse, int* err) {
  if (blockIdx.x != 0) return;
  k_page_extract_body(page, page_len, out, nvals, src_esz, has_def,
                      flba_reverse, nullptr, nullptr, err);
}

extern "C" int bg_page_extract(const void* d_page, int64_t page_len,
                               void* d_out, int64_t dst_byte_off,
                               int64_t nvals, int64_t src_esz,
                               int32_t has_def, int32_t flba_reverse) {
  REQUIRE_INIT();
  DevBuf<int> d_err;
  HIP_TRY(d_err.alloc(1));
  HIP_TRY(hipMemset(d_err, 0, sizeof(int)));
  int blocks = (int)bg_imin64((nvals * src_esz + BG_BLOCK - 1) / BG_BLOCK, 512);
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL(k_page_extract, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (const uint8_t*)d_page, page_len,
                     (uint8_t*)d_out + dst_byte_off, nvals, src_esz, has_def,
                     flba_reverse, d_err);
  HIP_TRY(hipGetLastError());
  int err = 0;
  HIP_TRY(hipMemcpy(&err, d_err, sizeof(int), hipMemcpyDeviceToHost));
  if (err)
    return set_err(BG_ERR_UNSUPPORTED,
                   "bg_page_extract: page carries nulls or malformed def "
                   "levels (null decode: later round)");
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Parquet dictionary-encoded data pages (PLAIN_DICTIONARY/RLE_DICTIONARY —
// the default layout modern writers produce): after the def-level block the
// page holds [u8 bit_width][RLE/bit-packed hybrid dictionary indices].
// One thread expands one page's indices serially (strictly byte-serial
// format; pages decode concurrently); the column is then materialised with
// the existing bg_gather from the (PLAIN-decoded) dictionary.
// ---------------------------------------------------------------------------
// Wave-cooperative index expansion: lane 0 parses the serial headers
// (def levels + hybrid run headers) and broadcasts; all 64 lanes expand
// bit-packed groups (one group of 8 per lane) and RLE fills in parallel.
__device__ void k_dict_indices_body(const uint8_t* page, int64_t page_len,
                                    int64_t nvals, int has_def,
                                    uint32_t* out_idx, const uint32_t* vidx,
                                    const int64_t* n_present, uint32_t* dense,
                                    int* err) {
  const int lane = lane_id();
  const int64_t nslots = nvals;
  uint32_t* const slots_out = out_idx;
  if (has_def == 2) {
    // nullable: the packed index stream holds n_present entries; decode
    // them densely into `dense`, then scatter to slots through vidx
    // (NULL slots get index 0 — a valid dictionary read whose value the
    // validity bitmap masks, matching the reference's null-padded take)
    nvals = *n_present;
    out_idx = dense;
  }
  int64_t doff = 0;
  int ok = 1;
  int bw = 0;
  if (lane == 0) {
    const uint8_t* d = page;
    if (has_def == 2) {
      if (page_len < 4) ok = 0;
      else {
        const uint32_t dlen = (uint32_t)d[0] | ((uint32_t)d[1] << 8) |
                              ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24);
        doff = 4 + (int64_t)dlen;
        if (doff > page_len) ok = 0;
      }
    } else if (has_def) {
      if (page_len < 4) ok = 0;
      else {
        const uint32_t dlen = (uint32_t)d[0] | ((uint32_t)d[1] << 8) |
                              ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24);
        const uint8_t* dl = d + 4;
        if ((int64_t)dlen > page_len - 4) ok = 0;
        const uint8_t* dlend = ok ? dl + dlen : dl;
        int64_t seen = 0;
        while (ok && dl < dlend && seen < nvals) {
          u64 header = 0;
          if (!bg_uvarint(dl, dlend, &header)) { ok = 0; break; }
          if (header & 1) {
            const int64_t groups = (int64_t)(header >> 1);
            for (int64_t g = 0; g < groups && ok; ++g) {
              if (dl >= dlend) { ok = 0; break; }
              const uint8_t byte = *dl++;
              const int64_t take = nvals - seen >= 8 ? 8 : nvals - seen;
              for (int64_t t = 0; t < take; ++t)
                if (!((byte >> t) & 1)) ok = 0;
              seen += take;
            }
          } else {
            const int64_t run = (int64_t)(header >> 1);
            if (dl >= dlend || *dl++ != 1) ok = 0;
            seen += run < nvals - seen ? run : nvals - seen;
          }
        }
        if (seen < nvals) ok = 0;
        doff = 4 + (int64_t)dlen;
      }
    }
    if (ok) {
      if (doff >= page_len) ok = 0;
      else {
        bw = page[doff];
        doff += 1;
        if (bw < 0 || bw > 32) ok = 0;
      }
    }
  }
  ok = bcast32(ok);
  bw = bcast32(bw);
  doff = bcast64(doff);
  if (!ok) {
    if (lane == 0) atomicExch(err, 2);
    return;
  }
  if (bw == 0) {
    for (int64_t t = lane; t < nslots; t += BG_WAVE) slots_out[t] = 0;
    return;
  }
  const u64 vmask = (bw == 32) ? 0xffffffffull : ((1ull << bw) - 1);
  int64_t outp = 0;
  int64_t si = doff;
  while (outp < nvals) {
    // lane 0 parses one run header
    u64 header = 0;
    int hok = 1;
    int64_t nsi = si;
    u64 rle_val = 0;
    if (lane == 0) {
      const uint8_t* hp = page + nsi;
      if (!bg_uvarint(hp, page + page_len, &header)) hok = 0;
      nsi = hp - page;
      if (hok && !(header & 1)) {
        const int nb = (bw + 7) / 8;
        if (nsi + nb > page_len) hok = 0;
        else {
          for (int b2 = 0; b2 < nb; ++b2)
            rle_val |= (u64)page[nsi + b2] << (8 * b2);
          nsi += nb;
        }
      }
    }
    hok = bcast32(hok);
    if (!hok) { if (lane == 0) atomicExch(err, 3); return; }
    header = (u64)bcast64((int64_t)header);
    nsi = bcast64(nsi);
    rle_val = (u64)bcast64((int64_t)rle_val);
    if (header & 1) {  // bit-packed: ngroups groups of 8, bw bytes each
      const int64_t groups = (int64_t)(header >> 1);
      // (page_len - nsi) / bw, not groups * bw: a hostile count overflows
      if (groups > (page_len - nsi) / bw) {
        if (lane == 0) atomicExch(err, 3);
        return;
      }
      // lane L expands group (gb + L)
      for (int64_t gb = 0; gb < groups; gb += BG_WAVE) {
        const int64_t g = gb + lane;
        if (g < groups) {
          const uint8_t* gp = page + nsi + g * bw;
          const int64_t base_out = outp + g * 8;
          const int64_t take = nvals - base_out >= 8
                                   ? 8
                                   : (nvals > base_out ? nvals - base_out : 0);
          for (int64_t t = 0; t < take; ++t) {
            const int bitpos = (int)(t * bw);
            const int bytepos = bitpos >> 3;
            const int shift2 = bitpos & 7;
            u64 w = 0;
            const int avail = bw - bytepos;
            const int nload = avail < 8 ? avail : 8;
            for (int b2 = 0; b2 < nload; ++b2)
              w |= (u64)gp[bytepos + b2] << (8 * b2);
            out_idx[base_out + t] = (uint32_t)((w >> shift2) & vmask);
          }
        }
      }
      const int64_t produced = groups * 8;
      outp += produced < nvals - outp ? produced : nvals - outp;
      si = nsi + groups * bw;
    } else {  // RLE run: parallel fill
      const int64_t run = (int64_t)(header >> 1);
      const int64_t take = run <= nvals - outp ? run : nvals - outp;
      for (int64_t t = lane; t < take; t += BG_WAVE)
        out_idx[outp + t] = (uint32_t)rle_val;
      outp += take;
      si = nsi;
    }
  }
  if (has_def == 2) {
    __builtin_amdgcn_wave_barrier();
    for (int64_t t = lane; t < nslots; t += BG_WAVE) {
      const uint32_t ix = vidx[t];
      slots_out[t] = (ix == 0xffffffffu) ? 0u : dense[ix];
    }
  }
}

__global__ void k_dict_indices(const uint8_t* page, int64_t page_len,
                               int64_t nvals, int has_def, uint32_t* out_idx,
                               int* err) {
  if (blockIdx.x != 0 || threadIdx.x >= BG_WAVE) return;
  k_dict_indices_body(page, page_len, nvals, has_def, out_idx, nullptr,
                      nullptr, nullptr, err);
}

extern "C" int bg_dict_indices(const void* d_page, int64_t page_len,
                               int64_t nvals, int32_t has_def,
                               uint32_t* d_out_idx) {
  REQUIRE_INIT();
  DevBuf<int> d_err;
  HIP_TRY(d_err.alloc(1));
  HIP_TRY(hipMemset(d_err, 0, sizeof(int)));
  hipLaunchKernelGGL(k_dict_indices, dim3(1), dim3(64), 0, 0,
                     (const uint8_t*)d_page, page_len, nvals, has_def,
                     d_out_idx, d_err);
  HIP_TRY(hipGetLastError());
  int err = 0;
  HIP_TRY(hipMemcpy(&err, d_err, sizeof(int), hipMemcpyDeviceToHost));
  if (err == 2)
    return set_err(BG_ERR_UNSUPPORTED, "bg_dict_indices: nulls (later round)");
  if (err)
    return set_err(BG_ERR_INVALID, "bg_dict_indices: malformed index block");
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Definition-level decode for OPTIONAL (nullable) columns: parquet data
// pages of a max_def=1 column prefix the payload with [u32 len][RLE/bit-
// packed bit-width-1 levels]; level 1 = value present, 0 = NULL (format
// restated from the parquet-format spec Encodings.md, the same hybrid the
// reference's parquet crate decodes in
// parquet/src/encodings/rle.rs).  Lane 0 walks one page's levels serially
// (pages decode concurrently across waves), emitting
//   - the column's Arrow LSB validity bits (atomicOr into u32 words at an
//     arbitrary bit offset — page boundaries are not byte-aligned),
//   - vidx[s] = index of slot s's value in the page's packed value
//     stream (~0u for NULL slots),
//   - n_present = how many values the page's value section holds.
// ---------------------------------------------------------------------------
__device__ void k_def_levels_body(const bg_def_levels_job& job, int* err) {
  if (lane_id() != 0) return;
  const uint8_t* page = job.d_page;
  if (job.page_len < 4) { atomicExch(err, 3); return; }
  const uint32_t dlen = (uint32_t)page[0] | ((uint32_t)page[1] << 8) |
                        ((uint32_t)page[2] << 16) | ((uint32_t)page[3] << 24);
  if ((int64_t)dlen > job.page_len - 4) { atomicExch(err, 3); return; }
  const uint8_t* d = page + 4;
  const uint8_t* dend = d + dlen;
  int64_t s = 0;        // slot
  uint32_t cnt = 0;     // values seen
  int64_t cur_w = -1;   // current validity word index
  uint32_t cur = 0;
  auto emit = [&](int present) {
    const int64_t bit = job.bit_off + s;
    const int64_t w = bit >> 5;
    if (w != cur_w) {
      if (cur_w >= 0 && cur) atomicOr(&job.d_valid_out[cur_w], cur);
      cur_w = w;
      cur = 0;
    }
    if (present) {
      cur |= 1u << (bit & 31);
      job.d_vidx[s] = cnt++;
    } else {
      job.d_vidx[s] = 0xffffffffu;
    }
    ++s;
  };
  while (d < dend && s < job.nvals) {
    u64 header = 0;
    if (!bg_uvarint(d, dend, &header)) { atomicExch(err, 3); return; }
    if (header & 1) {  // bit-packed groups of 8, 1 byte each (bit width 1)
      const int64_t groups = (int64_t)(header >> 1);
      for (int64_t g = 0; g < groups && s < job.nvals; ++g) {
        if (d >= dend) { atomicExch(err, 3); return; }
        const uint8_t byte = *d++;
        const int64_t take = job.nvals - s >= 8 ? 8 : job.nvals - s;
        for (int64_t t = 0; t < take; ++t) emit((byte >> t) & 1);
      }
    } else {  // RLE run
      const int64_t run = (int64_t)(header >> 1);
      if (d >= dend) { atomicExch(err, 3); return; }
      const int v = *d++ & 1;
      for (int64_t t = 0; t < run && s < job.nvals; ++t) emit(v);
    }
  }
  if (cur_w >= 0 && cur) atomicOr(&job.d_valid_out[cur_w], cur);
  if (s < job.nvals) { atomicExch(err, 3); return; }
  *job.d_n_present = (int64_t)cnt;
}

__global__ void k_def_levels_batch(const bg_def_levels_job* jobs, int64_t njobs,
                                   int* err) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t j = wave_global; j < njobs; j += nwaves)
    k_def_levels_body(jobs[j], err);
}

extern "C" int bg_def_levels_batch(const bg_def_levels_job* h_jobs,
                                   int64_t njobs) {
  REQUIRE_INIT();
  int err = 0;
  if (int rc = run_job_batch(
          k_def_levels_batch, h_jobs, njobs,
          grid_for(njobs, BG_BLOCK / BG_WAVE), &err))
    return rc;
  if (err)
    return set_err(BG_ERR_INVALID, "bg_def_levels_batch: malformed levels");
  return BG_OK;
}

// ---------------------------------------------------------------------------
// LIST columns (parquet repetition levels, max_rep == 1): a V1 page body
// is [u32 rlen][rep levels][u32 dlen][def levels][values].  rep == 0
// starts a row; def tells how far down the schema the slot is defined
// (0 = NULL list, 1 = empty list, >= def_entry = an element slot exists,
// == max_def = the element is non-null and consumes one packed value).
// Rows never span pages (checked), so one wave-lane walks both level
// streams per page: pass 1 counts {rows, entries, present} and reports
// rlen (the host needs it to re-point the UNCHANGED extract/dict kernels
// at the [u32 dlen][def][values] suffix); pass 2 emits per-row entry
// counts, the two validity bitmaps and the page-local value index per
// entry (the same vidx contract bg_def_levels_batch feeds mode-2
// extraction with).  Levels are the RLE/bit-packed hybrid at bit width
// <= 8 (max_def <= 255); deeper nesting (max_rep > 1) is rejected by the
// host reader.
// ---------------------------------------------------------------------------
struct LvlRd {
  const uint8_t* d;
  const uint8_t* end;
  int w;
  int64_t rle_left = 0;
  int rle_val = 0;
  int64_t bp_left = 0;
  int64_t bp_bytes = 0;  // bytes remaining in the current bit-packed run
  u64 bitbuf = 0;
  int bits = 0;
  bool ok = true;
  __device__ int next() {
    while (true) {
      if (rle_left > 0) {
        --rle_left;
        return rle_val;
      }
      if (bp_left > 0) {
        if (bits < w) {
          // refill ONLY from this run's own bytes — reading ahead would
          // swallow the next run's header
          while (bits <= 56 && bp_bytes > 0 && d < end) {
            bitbuf |= (u64)(*d++) << bits;
            bits += 8;
            --bp_bytes;
          }
          if (bits < w) {
            ok = false;
            return 0;
          }
        }
        const int v = (int)(bitbuf & ((1u << w) - 1));
        bitbuf >>= w;
        bits -= w;
        --bp_left;
        return v;
      }
      if (d >= end) {
        ok = false;
        return 0;
      }
      u64 h = 0;
      if (!bg_uvarint(d, end, &h)) {
        ok = false;
        return 0;
      }
      if (h & 1) {
        // the bytes left can feed fewer than (end - d + 1) groups, so the
        // clamp changes nothing but keeps a hostile count from overflowing
        const u64 avail = (u64)(end - d) + 1;
        const int64_t groups = (int64_t)((h >> 1) < avail ? (h >> 1) : avail);
        bp_left = groups * 8;  // groups of 8 w-bit values
        bp_bytes = groups * w;
        bitbuf = 0;
        bits = 0;
      } else {
        rle_left = (int64_t)(h >> 1);
        if (d >= end) {
          ok = false;
          return 0;
        }
        rle_val = *d++;  // bit width <= 8: value fits one byte
      }
    }
  }
};

__device__ __forceinline__ int bg_bitwidth(int v) {
  int w = 0;
  while ((1 << w) <= v) ++w;
  return w < 1 ? 1 : w;
}

__device__ void k_list_levels_body(const bg_list_levels_job& job, int pass,
                                   int* err) {
  if (lane_id() != 0) return;
  const uint8_t* page = job.d_page;
  const int64_t plen = job.page_len;
  if (plen < 8) { atomicExch(err, 4); return; }
  const uint32_t rlen = (uint32_t)page[0] | ((uint32_t)page[1] << 8) |
                        ((uint32_t)page[2] << 16) |
                        ((uint32_t)page[3] << 24);
  if (4 + (int64_t)rlen + 4 > plen) { atomicExch(err, 4); return; }
  const uint8_t* dpos = page + 4 + rlen;
  const uint32_t dlen = (uint32_t)dpos[0] | ((uint32_t)dpos[1] << 8) |
                        ((uint32_t)dpos[2] << 16) |
                        ((uint32_t)dpos[3] << 24);
  if (4 + (int64_t)rlen + 4 + (int64_t)dlen > plen) {
    atomicExch(err, 4);
    return;
  }
  LvlRd rr{page + 4, page + 4 + rlen, 1};
  LvlRd dr{dpos + 4, dpos + 4 + dlen, bg_bitwidth(job.max_def)};
  int64_t rows = 0, entries = 0, present = 0;
  int64_t cur_row = -1;
  // word-batched bitmap emission (same pattern as the def-level walk)
  int64_t lv_w = -1, ev_w = -1;
  uint32_t lv_cur = 0, ev_cur = 0;
  for (int64_t s = 0; s < job.nslots; ++s) {
    const int rep = rr.next();
    const int def = dr.next();
    if (!rr.ok || !dr.ok || rep > 1 || def > job.max_def) {
      atomicExch(err, 4);
      return;
    }
    if (s == 0 && rep != 0) {  // a row spanning pages: unsupported
      atomicExch(err, 5);
      return;
    }
    if (rep == 0) {
      cur_row = job.row_base + rows;
      ++rows;
      if (pass == 2) {
        job.d_row_sizes[cur_row] = 0;
        if (def >= job.def_valid) {
          const int64_t w = cur_row >> 5;
          if (w != lv_w) {
            if (lv_w >= 0 && lv_cur) atomicOr(&job.d_list_valid[lv_w], lv_cur);
            lv_w = w;
            lv_cur = 0;
          }
          lv_cur |= 1u << (cur_row & 31);
        }
      }
    }
    if (def >= job.def_entry) {
      if (pass == 2) {
        const int64_t ent = job.entry_base + entries;
        job.d_row_sizes[cur_row] += 1;
        if (def == job.max_def) {
          const int64_t w = ent >> 5;
          if (w != ev_w) {
            if (ev_w >= 0 && ev_cur) atomicOr(&job.d_elem_valid[ev_w], ev_cur);
            ev_w = w;
            ev_cur = 0;
          }
          ev_cur |= 1u << (ent & 31);
          job.d_vidx[entries] = (uint32_t)present;
        } else {
          job.d_vidx[entries] = 0xffffffffu;
        }
      }
      ++entries;
    }
    if (def == job.max_def) ++present;
  }
  if (pass == 2) {
    if (lv_w >= 0 && lv_cur) atomicOr(&job.d_list_valid[lv_w], lv_cur);
    if (ev_w >= 0 && ev_cur) atomicOr(&job.d_elem_valid[ev_w], ev_cur);
  } else {
    job.d_counts[0] = rows;
    job.d_counts[1] = entries;
    job.d_counts[2] = present;
    job.d_counts[3] = (int64_t)rlen;
  }
}

__global__ void k_list_levels_batch(const bg_list_levels_job* jobs,
                                    int64_t njobs, int pass, int* err) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t j = wave_global; j < njobs; j += nwaves)
    k_list_levels_body(jobs[j], pass, err);
}

extern "C" int bg_list_levels_batch(const bg_list_levels_job* h_jobs,
                                    int64_t njobs, int32_t pass) {
  REQUIRE_INIT();
  if (njobs <= 0) return BG_OK;
  int err = 0;
  if (int rc = run_job_batch(
          k_list_levels_batch, h_jobs, njobs,
          grid_for(njobs, BG_BLOCK / BG_WAVE), &err, (int)pass))
    return rc;
  if (err == 5)
    return set_err(BG_ERR_UNSUPPORTED,
                   "bg_list_levels_batch: row spans pages");
  if (err)
    return set_err(BG_ERR_INVALID, "bg_list_levels_batch: malformed levels");
  return BG_OK;
}

// ---------------------------------------------------------------------------
// DELTA_BINARY_PACKED (encoding 5) integer pages — the reference's
// parquet-rs V2 writer default for INT32/INT64 (restated from the parquet
// spec Encodings.md "Delta Encoding"): header = <block_size varint>
// <miniblocks_per_block varint> <total_count varint> <first zigzag>;
// per block: <min_delta zigzag> <bit widths, 1 B per miniblock>
// <packed miniblocks>; value[i+1] = value[i] + min_delta + delta[i].
// Lane 0 walks one page serially (the prefix chain is inherently
// sequential); pages decode concurrently across waves.  Nullable slots
// scatter through vidx like the other extractors.
// ---------------------------------------------------------------------------
// Reusable serial reader for one DELTA_BINARY_PACKED integer stream
// (consumed by encodings 5, 6 and 7).  One lane; returns false on
// malformed input.  After `count` values, `p` rests at the first byte
// past the stream (writers pad the final miniblock to full width).
struct DbpStream {
  const uint8_t* p;
  const uint8_t* pend;
  u64 block_size = 0, mb_per_block = 0, total = 0;
  int64_t mb_vals = 0;
  i64 value = 0;     // last emitted value
  i64 min_delta = 0;
  const uint8_t* bws = nullptr;  // current block's bit widths
  u64 mb = 0;        // miniblock index within block (mb_per_block = fresh)
  int64_t t = 0;     // value index within miniblock
  int64_t produced = 0;
  int bw = 0;
  int64_t mb_bytes = 0;

  __device__ bool varint(u64* out_v) { return bg_uvarint(p, pend, out_v); }
  __device__ bool zigzag(i64* out_v) {
    u64 v;
    if (!varint(&v)) return false;
    *out_v = (i64)(v >> 1) ^ -(i64)(v & 1);
    return true;
  }
  __device__ bool init(const uint8_t* start, const uint8_t* end) {
    p = start;
    pend = end;
    i64 first;
    if (!varint(&block_size) || !varint(&mb_per_block) || !varint(&total) ||
        !zigzag(&first))
      return false;
    if (!mb_per_block || !block_size || block_size % mb_per_block)
      return false;
    // a page header counts values in an i32: a larger block is malformed,
    // and the bound keeps bw * mb_vals below from overflowing
    if (block_size > 0x7fffffffull) return false;
    mb_vals = (int64_t)(block_size / mb_per_block);
    // the spec asks for a multiple of 32; bw * mb_vals / 8 below is a whole
    // byte count only for a multiple of 8
    if (mb_vals % 8) return false;
    value = first;
    mb = mb_per_block;  // force new block on first next_after_first
    t = 0;
    produced = 1;       // `value` holds the first value already
    return true;
  }
  // advance to the next value (call total-1 times after init)
  __device__ bool next() {
    if (t >= mb_vals) { t = 0; p += mb_bytes; ++mb; }
    if (mb >= mb_per_block) {
      if (!zigzag(&min_delta)) return false;
      if (mb_per_block > (u64)(pend - p)) return false;
      bws = p;
      p += mb_per_block;
      mb = 0;
      t = 0;
    }
    if (t == 0) {
      bw = bws[mb];
      if (bw > 64) return false;
      mb_bytes = (int64_t)bw * mb_vals / 8;
      if (mb_bytes > pend - p) return false;
    }
    u64 d = 0;
    if (bw) {
      const int64_t bit = t * bw;
      const int64_t byte = bit >> 3;
      const int sh = (int)(bit & 7);
      // bw + sh can exceed 64 (full-width deltas off a bit boundary):
      // assemble through u128 so no high bits are lost
      u128 acc = 0;
      for (int b2 = 0; b2 * 8 < bw + sh; ++b2)
        if (byte + b2 < mb_bytes) acc |= (u128)p[byte + b2] << (8 * b2);
      d = (u64)(acc >> sh);
      if (bw < 64) d &= (1ull << bw) - 1;
    }
    ++t;
    // the spec's arithmetic wraps: add in u64, signed overflow is undefined
    value = (i64)((u64)value + (u64)min_delta + d);
    ++produced;
    return true;
  }
  // position p just past the stream (after consuming exactly `total`)
  __device__ bool finish() {
    while (produced < (int64_t)total)
      if (!next()) return false;
    if (t > 0 || total == 1) p += mb_bytes;  // skip the last miniblock data
    return true;
  }
};

__device__ void k_delta_bp_body(const bg_delta_bp_job& job, int* err) {
  if (lane_id() != 0) return;
  const uint8_t* p = job.d_page;
  const uint8_t* pend = p + job.page_len;
  if (job.has_def) {
    if (job.page_len < 4) { atomicExch(err, 3); return; }
    const uint32_t dlen = (uint32_t)p[0] | ((uint32_t)p[1] << 8) |
                          ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    if ((int64_t)dlen > job.page_len - 4) { atomicExch(err, 3); return; }
    p += 4 + dlen;
  }
  DbpStream st;
  if (!st.init(p, pend)) { atomicExch(err, 3); return; }
  const int64_t want = job.has_def == 2 ? *job.d_n_present : job.nvals;
  if ((int64_t)st.total < want || want == 0) {
    if (want != 0) atomicExch(err, 3);
    return;
  }
  int64_t slot = 0;
  auto emit = [&](i64 v) {
    if (job.has_def == 2)
      while (slot < job.nvals && job.d_vidx[slot] == 0xffffffffu) ++slot;
    if (slot < job.nvals) {
      if (job.esz == 8)
        *(int64_t*)(job.d_out + slot * 8) = v;
      else
        *(int32_t*)(job.d_out + slot * 4) = (int32_t)v;
      ++slot;
    }
  };
  emit(st.value);
  for (int64_t k2 = 1; k2 < want; ++k2) {
    if (!st.next()) { atomicExch(err, 3); return; }
    emit(st.value);
  }
}

// DELTA_LENGTH_BYTE_ARRAY (6): one DBP stream of lengths, then the
// concatenated bytes — lengths + absolute source addresses feed the
// shared bg_ba_materialize path.  DELTA_BYTE_ARRAY (7): DBP prefix
// lengths + DBP suffix lengths + suffix bytes; pass 1 records total
// lengths (srcaddr 0 = "reconstructed later"), pass 2 rebuilds each
// string from its predecessor's prefix + its suffix at the final
// offsets (lane-0 serial per page; strings share prefixes only within
// a page).
__device__ void k_delta_ba_body(const bg_delta_ba_job& job, int pass,
                                int* err) {
  if (lane_id() != 0) return;
  const uint8_t* p = job.d_page;
  const uint8_t* pend = p + job.page_len;
  if (job.has_def) {
    if (job.page_len < 4) { atomicExch(err, 3); return; }
    const uint32_t dlen = (uint32_t)p[0] | ((uint32_t)p[1] << 8) |
                          ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    if ((int64_t)dlen > job.page_len - 4) { atomicExch(err, 3); return; }
    p += 4 + dlen;
  }
  const int64_t want = job.has_def == 2 ? *job.d_n_present : job.nvals;
  if (pass == 1)
    for (int64_t t = 0; t < job.nvals; ++t) {
      job.d_lens_out[t] = 0;
      job.d_srcaddr_out[t] = 0;
    }
  if (want == 0) return;
  if (job.enc == 6) {
    DbpStream lens;
    if (!lens.init(p, pend) || (int64_t)lens.total < want) {
      atomicExch(err, 3);
      return;
    }
    // walk lengths; bytes follow the stream — position after via finish()
    // (needs a second pass over the stream: re-init and emit)
    DbpStream probe = lens;
    if (!probe.finish()) { atomicExch(err, 3); return; }
    const uint8_t* bytes = probe.p;
    int64_t slot = 0, cursor = 0;
    // a negative length, or one past the page's bytes, is rejected before
    // it reaches the scan in bg_ba_materialize
    auto emit = [&](i64 ln) -> bool {
      if (ln < 0 || ln > (pend - bytes) - cursor) return false;
      if (job.has_def == 2)
        while (slot < job.nvals && job.d_vidx[slot] == 0xffffffffu) ++slot;
      if (slot < job.nvals) {
        job.d_lens_out[slot] = ln;
        job.d_srcaddr_out[slot] = (int64_t)(uintptr_t)(bytes + cursor);
        ++slot;
      }
      cursor += ln;
      return true;
    };
    if (!emit(lens.value)) { atomicExch(err, 3); return; }
    for (int64_t k2 = 1; k2 < want; ++k2) {
      if (!lens.next() || !emit(lens.value)) { atomicExch(err, 3); return; }
    }
    return;
  }
  // enc 7: prefix lens stream, suffix lens stream, suffix bytes
  DbpStream pre;
  if (!pre.init(p, pend) || (int64_t)pre.total < want) {
    atomicExch(err, 3);
    return;
  }
  DbpStream pre_probe = pre;
  if (!pre_probe.finish()) { atomicExch(err, 3); return; }
  DbpStream suf;
  if (!suf.init(pre_probe.p, pend) || (int64_t)suf.total < want) {
    atomicExch(err, 3);
    return;
  }
  DbpStream suf_probe = suf;
  if (!suf_probe.finish()) { atomicExch(err, 3); return; }
  const uint8_t* sbytes = suf_probe.p;
  int64_t slot = 0, cursor = 0;
  int64_t prev_off = -1;  // output offset of the previous string (pass 2)
  int64_t prev_len = 0;
  bool first = true;
  auto step = [&](i64 plen, i64 slen) -> bool {
    if (plen < 0 || slen < 0) return false;
    if (slen > (pend - sbytes) - cursor) return false;  // suffix past page
    if (first && plen != 0) return false;  // nothing to prefix from
    if (!first && plen > prev_len) return false;
    if (job.has_def == 2)
      while (slot < job.nvals && job.d_vidx[slot] == 0xffffffffu) ++slot;
    if (slot < job.nvals) {
      if (pass == 1) {
        job.d_lens_out[slot] = plen + slen;
        // srcaddr stays 0: k_ba_copy skips, pass 2 reconstructs
      } else {
        const int64_t off = (int64_t)job.d_offs32[slot];
        uint8_t* dst = job.d_data_out + off;
        if (!first)
          for (int64_t b = 0; b < plen; ++b)
            dst[b] = job.d_data_out[prev_off + b];
        for (int64_t b = 0; b < slen; ++b) dst[plen + b] = sbytes[cursor + b];
        prev_off = off;
      }
      prev_len = plen + slen;  // both passes: the prefix bound check
      ++slot;
    }
    cursor += slen;
    first = false;
    return true;
  };
  if (!step(pre.value, suf.value)) { atomicExch(err, 3); return; }
  for (int64_t k2 = 1; k2 < want; ++k2) {
    if (!pre.next() || !suf.next()) { atomicExch(err, 3); return; }
    if (!step(pre.value, suf.value)) { atomicExch(err, 3); return; }
  }
  if (sbytes + cursor > pend) atomicExch(err, 3);
}

__global__ void k_delta_ba_batch(const bg_delta_ba_job* jobs, int64_t njobs,
                                 int pass, int* err) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t j = wave_global; j < njobs; j += nwaves)
    k_delta_ba_body(jobs[j], pass, err);
}

extern "C" int bg_delta_ba_batch(const bg_delta_ba_job* h_jobs, int64_t njobs,
                                 int32_t pass) {
  REQUIRE_INIT();
  int err = 0;
  if (int rc = run_job_batch(
          k_delta_ba_batch, h_jobs, njobs,
          grid_for(njobs, BG_BLOCK / BG_WAVE), &err, (int)pass))
    return rc;
  if (err)
    return set_err(BG_ERR_INVALID, "bg_delta_ba_batch: malformed page");
  return BG_OK;
}

__global__ void k_delta_bp_batch(const bg_delta_bp_job* jobs, int64_t njobs,
                                 int* err) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t j = wave_global; j < njobs; j += nwaves)
    k_delta_bp_body(jobs[j], err);
}

extern "C" int bg_delta_bp_batch(const bg_delta_bp_job* h_jobs, int64_t njobs) {
  REQUIRE_INIT();
  int err = 0;
  if (int rc = run_job_batch(
          k_delta_bp_batch, h_jobs, njobs,
          grid_for(njobs, BG_BLOCK / BG_WAVE), &err))
    return rc;
  if (err)
    return set_err(BG_ERR_INVALID, "bg_delta_bp_batch: malformed page");
  return BG_OK;
}

// ---------------------------------------------------------------------------
// BYTE_ARRAY (Utf8/Binary) PLAIN page extraction: the value section is a
// byte-serial [u32 len][bytes] sequence (parquet spec Encodings.md PLAIN;
// the reference decodes it in parquet/src/encodings/decoding.rs).  Lane 0
// walks one page serially recording each slot's length and absolute source
// address (pages decode concurrently); the column then materialises with
// one exclusive scan over the lengths + a parallel copy
// (bg_ba_materialize) into Arrow offsets+data form.
// ---------------------------------------------------------------------------
__device__ void k_ba_extract_body(const bg_ba_page_job& job, int* err) {
  const int lane = lane_id();
  for (int64_t t = lane; t < job.nvals; t += BG_WAVE) {
    job.d_lens_out[t] = 0;
    job.d_srcaddr_out[t] = 0;
  }
  __builtin_amdgcn_wave_barrier();
  if (lane != 0) return;
  const uint8_t* p = job.d_page;
  int64_t pos = 0;
  if (job.has_def) {
    if (job.page_len < 4) { atomicExch(err, 3); return; }
    const uint32_t dlen = (uint32_t)p[0] | ((uint32_t)p[1] << 8) |
                          ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    pos = 4 + (int64_t)dlen;
    if (pos > job.page_len) { atomicExch(err, 3); return; }
  }
  for (int64_t s = 0; s < job.nvals; ++s) {
    if (job.has_def == 2 && job.d_vidx[s] == 0xffffffffu) continue;
    if (pos + 4 > job.page_len) { atomicExch(err, 3); return; }
    const uint32_t len = (uint32_t)p[pos] | ((uint32_t)p[pos + 1] << 8) |
                         ((uint32_t)p[pos + 2] << 16) |
                         ((uint32_t)p[pos + 3] << 24);
    pos += 4;
    if (pos + (int64_t)len > job.page_len) { atomicExch(err, 3); return; }
    job.d_lens_out[s] = (int64_t)len;
    job.d_srcaddr_out[s] = (int64_t)(uintptr_t)(p + pos);
    pos += (int64_t)len;
  }
}

__global__ void k_ba_extract_batch(const bg_ba_page_job* jobs, int64_t njobs,
                                   int* err) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t j = wave_global; j < njobs; j += nwaves)
    k_ba_extract_body(jobs[j], err);
}

extern "C" int bg_ba_extract_batch(const bg_ba_page_job* h_jobs,
                                   int64_t njobs) {
  REQUIRE_INIT();
  int err = 0;
  if (int rc = run_job_batch(
          k_ba_extract_batch, h_jobs, njobs,
          grid_for(njobs, BG_BLOCK / BG_WAVE), &err))
    return rc;
  if (err)
    return set_err(BG_ERR_INVALID, "bg_ba_extract_batch: malformed page");
  return BG_OK;
}

// dict-coded BYTE_ARRAY pages: slot lengths/addresses come from the
// PLAIN-decoded dictionary through the expanded indices (NULL slots -> 0)
__global__ void k_ba_from_dict(const uint32_t* idx, const int32_t* doffs,
                               const uint8_t* ddata, const uint32_t* vidx,
                               int64_t n, int64_t* lens_out,
                               int64_t* srcaddr_out) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    if (vidx && vidx[s] == 0xffffffffu) {
      lens_out[s] = 0;
      srcaddr_out[s] = 0;
      continue;
    }
    const uint32_t ix = idx[s];
    const int32_t o = doffs[ix];
    lens_out[s] = (int64_t)(doffs[ix + 1] - o);
    srcaddr_out[s] = (int64_t)(uintptr_t)(ddata + o);
  }
}

extern "C" int bg_ba_from_dict(const uint32_t* d_idx, const int32_t* d_doffs,
                               const void* d_ddata, const uint32_t* d_vidx,
                               int64_t n, int64_t* d_lens_out,
                               int64_t* d_srcaddr_out) {
  REQUIRE_INIT();
  int blocks = grid_for(n);
  hipLaunchKernelGGL(k_ba_from_dict, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     d_idx, d_doffs, (const uint8_t*)d_ddata, d_vidx, n,
                     d_lens_out, d_srcaddr_out);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// scan lens -> Arrow i32 offsets (+ total) and copy every slot's bytes
__global__ void k_ba_copy(const int64_t* srcaddr, const int64_t* offs64,
                          int32_t* offs32, uint8_t* data, int64_t n) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = offs64[s];
    offs32[s] = (int32_t)o;
    const int64_t len = offs64[s + 1] - o;
    const uint8_t* src = (const uint8_t*)(uintptr_t)srcaddr[s];
    if (!src) continue;  // DELTA_BYTE_ARRAY slots: rebuilt by pass 2
    for (int64_t b = 0; b < len; ++b) data[o + b] = src[b];
  }
}

extern "C" int bg_ba_materialize(const int64_t* d_lens,
                                 const int64_t* d_srcaddr, int64_t n,
                                 int32_t* d_offs32 /* n+1 */,
                                 uint8_t* d_data /* total bytes */,
                                 int64_t data_cap, int64_t* out_total) {
  REQUIRE_INIT();
  DevBuf<i64> d_offs64;
  DevBuf<i64> d_total;
  HIP_TRY(d_offs64.alloc(n + 1));
  HIP_TRY(d_total.alloc(1));
  {
    int rc = scan_exclusive_i64((const u64*)d_lens, n, d_offs64, d_total);
    if (rc != BG_OK) return rc;
  }
  i64 total = 0;
  HIP_TRY(hipMemcpy(&total, d_total, sizeof(i64), hipMemcpyDeviceToHost));
  if (d_data == nullptr) {  // dry-run: size query only
    *out_total = total;
    return BG_OK;
  }
  if (total > data_cap || total > 0x7fffffffLL)
    return set_err(BG_ERR_INVALID, "bg_ba_materialize: data_cap/2GiB bound");
  HIP_TRY(hipMemcpy(d_offs64 + n, &total, sizeof(i64),
                    hipMemcpyHostToDevice));
  int blocks = grid_for(n);
  hipLaunchKernelGGL(k_ba_copy, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     d_srcaddr, (const int64_t*)d_offs64.get(), d_offs32, d_data,
                     n);
  HIP_TRY(hipGetLastError());
  const int32_t t32 = (int32_t)total;
  HIP_TRY(hipMemcpy(d_offs32 + n, &t32, sizeof(int32_t),
                    hipMemcpyHostToDevice));
  *out_total = total;
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Batched page ops: the per-page host loop (launch + sync error check per
// page) starves the GPU when chunks hold few pages — these take the whole
// column's page list in one call.
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// BYTE_STREAM_SPLIT (encoding 9, fixed-width values): the page stores the
// k-th byte of every value contiguously (k streams of n_present bytes) —
// a parallel byte transpose reassembles values; nullable slots scatter
// through vidx (spec Encodings.md; the reference's parquet crate
// byte_stream_split decoder).
// ---------------------------------------------------------------------------
__global__ void k_bss_batch(const bg_page_extract_job* jobs, int64_t njobs,
                            int* err) {
  for (int64_t j = blockIdx.x; j < njobs; j += gridDim.x) {
    const bg_page_extract_job job = jobs[j];
    const uint8_t* page = job.d_page;
    int64_t voff = 0;
    if (job.has_def) {
      if (job.page_len < 4) {
        if (threadIdx.x == 0) atomicExch(err, 3);
        continue;
      }
      const uint32_t dlen = (uint32_t)page[0] | ((uint32_t)page[1] << 8) |
                            ((uint32_t)page[2] << 16) |
                            ((uint32_t)page[3] << 24);
      voff = 4 + (int64_t)dlen;
    }
    const int64_t npres =
        job.has_def == 2 ? *job.d_n_present : job.nvals;
    if (voff + npres * job.src_esz > job.page_len) {
      if (threadIdx.x == 0) atomicExch(err, 3);
      continue;
    }
    const uint8_t* v = page + voff;
    for (int64_t s2 = threadIdx.x; s2 < job.nvals; s2 += blockDim.x) {
      int64_t k;
      if (job.has_def == 2) {
        const uint32_t ix = job.d_vidx[s2];
        if (ix == 0xffffffffu) continue;
        k = (int64_t)ix;
      } else {
        k = s2;
      }
      uint8_t* dst = job.d_out + s2 * job.src_esz;
      for (int64_t b = 0; b < job.src_esz; ++b)
        dst[b] = v[b * npres + k];
    }
  }
}

extern "C" int bg_bss_batch(const bg_page_extract_job* h_jobs, int64_t njobs) {
  REQUIRE_INIT();
  int err = 0;
  if (int rc = run_job_batch(
          k_bss_batch, h_jobs, njobs,
          grid_for(njobs, 1), &err))
    return rc;
  if (err) return set_err(BG_ERR_INVALID, "bg_bss_batch: malformed page");
  return BG_OK;
}

__global__ void k_page_extract_batch(const bg_page_extract_job* jobs,
                                     int64_t njobs, int* err) {
  for (int64_t j = blockIdx.x; j < njobs; j += gridDim.x) {
    const bg_page_extract_job job = jobs[j];
    k_page_extract_body(job.d_page, job.page_len, job.d_out, job.nvals,
                        job.src_esz, job.has_def, job.flba_reverse,
                        job.d_vidx, job.d_n_present, err);
  }
}

extern "C" int bg_page_extract_batch(const bg_page_extract_job* h_jobs,
                                     int64_t njobs) {
  REQUIRE_INIT();
  int err = 0;
  if (int rc = run_job_batch(
          k_page_extract_batch, h_jobs, njobs,
          grid_for(njobs, 1), &err))
    return rc;
  if (err)
    return set_err(BG_ERR_UNSUPPORTED,
                   "bg_page_extract_batch: nulls or malformed page");
  return BG_OK;
}

__global__ void k_dict_indices_batch(const bg_dict_indices_job* jobs,
                                     int64_t njobs, int* err) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t j = wave_global; j < njobs; j += nwaves) {
    const bg_dict_indices_job job = jobs[j];
    k_dict_indices_body(job.d_page, job.page_len, job.nvals, job.has_def,
                        job.d_out_idx, job.d_vidx, job.d_n_present, job.d_dense,
                        err);
  }
}

extern "C" int bg_dict_indices_batch(const bg_dict_indices_job* h_jobs,
                                     int64_t njobs) {
  REQUIRE_INIT();
  int err = 0;
  if (int rc = run_job_batch(
          k_dict_indices_batch, h_jobs, njobs,
          grid_for(njobs, BG_BLOCK / BG_WAVE), &err))
    return rc;
  if (err == 2)
    return set_err(BG_ERR_UNSUPPORTED, "bg_dict_indices_batch: nulls");
  if (err)
    return set_err(BG_ERR_INVALID, "bg_dict_indices_batch: malformed block");
  return BG_OK;
}

// Arrow offset rebase: partition slices of a shared i32 offsets vector
// start at arbitrary absolute byte positions — each partition's stream
// needs offsets rebased to 0 (the writer-side dual of read_partition's
// slice logic).
__global__ void k_sub_i32(const int32_t* src, int64_t n, int32_t sub,
                          int32_t* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = src[i] - sub;
}

extern "C" int bg_sub_i32(const void* d_src, int64_t n, int32_t sub,
                          void* d_out) {
  REQUIRE_INIT();
  int blocks = grid_for(n);
  hipLaunchKernelGGL(k_sub_i32, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (const int32_t*)d_src, n, sub, (int32_t*)d_out);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Variable-length (Utf8/Binary) row gather — the take/interleave the
// sort-shuffle writer needs for string payload columns
// (PartitionedBatchIterator handles every Arrow type).
// Two-phase: lengths -> exclusive scan -> wave-per-row byte copy.
// ---------------------------------------------------------------------------
__global__ void k_varlen_lens(const int32_t* src_offsets, const uint32_t* idx,
                              int64_t m, u64* lens) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t r = idx[i];
    lens[i] = (u64)(src_offsets[r + 1] - src_offsets[r]);
  }
}

__global__ void k_varlen_copy(const uint8_t* src_data,
                              const int32_t* src_offsets, const uint32_t* idx,
                              int64_t m, const i64* out_offs,
                              uint8_t* out_data, int32_t* out_offsets32) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  const int lane = lane_id();
  for (int64_t i = wave_global; i < m; i += nwaves) {
    const uint32_t r = idx[i];
    const int32_t lo = src_offsets[r];
    const int32_t len = src_offsets[r + 1] - lo;
    const i64 dst = out_offs[i];
    for (int32_t b = lane; b < len; b += BG_WAVE)
      out_data[dst + b] = src_data[lo + b];
    if (lane == 0) out_offsets32[i] = (int32_t)dst;
  }
}

__global__ void k_varlen_tail(int64_t m, const i64* total,
                              int32_t* out_offsets32) {
  if (blockIdx.x == 0 && threadIdx.x == 0) out_offsets32[m] = (int32_t)*total;
}

/* Gather m variable-length rows: writes Arrow i32 offsets (m+1) and packed
 * bytes; *out_total_bytes receives the data length (must fit i32 per Arrow
 * Utf8). */
extern "C" int bg_gather_varlen(const void* d_src_data,
                                const int32_t* d_src_offsets,
                                const uint32_t* d_idx, int64_t m,
                                int32_t* d_out_offsets /* m+1 */,
                                void* d_out_data, int64_t out_data_cap,
                                int64_t* out_total_bytes) {
  REQUIRE_INIT();
  DevBuf<u64> d_lens;
  DevBuf<i64> d_offs;
  DevBuf<i64> d_total;
  HIP_TRY(d_lens.alloc(m));
  HIP_TRY(d_offs.alloc(m));
  HIP_TRY(d_total.alloc(1));
  int blocks = grid_for(m);
  hipLaunchKernelGGL(k_varlen_lens, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     d_src_offsets, d_idx, m, d_lens);
  int rc = scan_exclusive_i64(d_lens, m, d_offs, d_total);
  if (rc != BG_OK) return rc;
  i64 total = 0;
  HIP_TRY(hipMemcpy(&total, d_total, sizeof(i64), hipMemcpyDeviceToHost));
  if (d_out_data == nullptr) {  // sizing call: report the needed bytes
    *out_total_bytes = total;
    return BG_OK;
  }
  if (total > out_data_cap)
    return set_err(BG_ERR_INVALID, "bg_gather_varlen: out_data too small");
  if (total > 0x7fffffffLL)
    return set_err(BG_ERR_INVALID,
                   "bg_gather_varlen: >2GiB Utf8 data (LargeUtf8: later)");
  const int waves_per_block = BG_BLOCK / BG_WAVE;
  int cblocks = grid_for(m, waves_per_block);
  hipLaunchKernelGGL(k_varlen_copy, dim3(cblocks), dim3(BG_BLOCK), 0, 0,
                     (const uint8_t*)d_src_data, d_src_offsets, d_idx, m,
                     d_offs, (uint8_t*)d_out_data, d_out_offsets);
  hipLaunchKernelGGL(k_varlen_tail, dim3(1), dim3(1), 0, 0, m, d_total,
                     d_out_offsets);
  HIP_TRY(hipGetLastError());
  *out_total_bytes = total;
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Validity-bitmap gather: out bit i = valid[idx[i]] — the take of a
// null-carrying column's validity buffer (Arrow LSB order; ballot word ==
// bitmap word).  Groundwork for nullable payload materialisation.
// ---------------------------------------------------------------------------
__global__ void k_gather_bits(const uint8_t* valid, const uint32_t* idx,
                              int64_t m, u64* out_words) {
  const int64_t nwords = (m + 63) / 64;
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t w = wave_global; w < nwords; w += nwaves) {
    const int64_t i = w * BG_WAVE + lane_id();
    bool bit = false;
    if (i < m) {
      const uint32_t r = idx[i];
      bit = (valid[r >> 3] >> (r & 7)) & 1;
    }
    const u64 word = __ballot(bit);
    if (lane_id() == 0) out_words[w] = word;
  }
}

extern "C" int bg_gather_bits(const uint8_t* d_valid, const uint32_t* d_idx,
                              int64_t m, uint8_t* d_out_bits) {
  REQUIRE_INIT();
  const int64_t nwords = (m + 63) / 64;
  const int waves_per_block = BG_BLOCK / BG_WAVE;
  int blocks = grid_for(nwords, waves_per_block);
  hipLaunchKernelGGL(k_gather_bits, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     d_valid, d_idx, m, reinterpret_cast<u64*>(d_out_bits));
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Device LZ4 block compression (SURVEY.md §8f row 3 — the GPU shuffle
// codec's compress half; decompression lives in k_snappy/... for parquet,
// and LZ4-frame DECODE is the CPU reader's job).  64 KiB blocks, one wave
// per block: lane 0 runs the greedy matcher (strictly serial emission)
// with a 4096-entry LDS hash table; blocks that don't shrink are reported
// as stored (negative size) and the host frames them uncompressed.
// Frame assembly (constant 7-byte header 04224d18/40/40/c0 + [u32 size]
// blocks + end mark) is host-side glue over the returned sizes.
// ---------------------------------------------------------------------------
#define LZ4_HASH_LOG 12

// wave-cooperative single-block compress; returns csize or -blen (stored)
__device__ int64_t lz4_compress_one(const uint8_t* s, int32_t blen,
                                    uint8_t* d, uint16_t* tab) {
  const int lane = lane_id();
  int64_t result = 0;
  {
    // parallel table clear (0xffff = empty)
    for (int i = lane; i < (1 << LZ4_HASH_LOG); i += BG_WAVE) tab[i] = 0xffff;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      int32_t pos = 0, anchor = 0, w = 0;
      const int32_t mflimit = blen - 12;  // no match may START past here
      const int32_t matchlimit = blen - 5;  // last 5 bytes stay literals
      bool overflow = false;
      auto emit_seq = [&](int32_t lit_len, int32_t mlen, int32_t moff) {
        // worst case bytes: 1 + lit_len/255+1 + lit_len + 2 + mlen/255+1
        if (w + lit_len + (lit_len / 255) + (mlen / 255) + 12 > blen) {
          overflow = true;
          return;
        }
        const int32_t ml_token = mlen >= 0 ? (mlen - 4) : 0;
        uint8_t token = (uint8_t)((lit_len < 15 ? lit_len : 15) << 4);
        if (mlen >= 0) token |= (uint8_t)(ml_token < 15 ? ml_token : 15);
        d[w++] = token;
        if (lit_len >= 15) {
          int32_t r = lit_len - 15;
          while (r >= 255) { d[w++] = 255; r -= 255; }
          d[w++] = (uint8_t)r;
        }
        for (int32_t i = 0; i < lit_len; ++i) d[w++] = s[anchor + i];
        if (mlen >= 0) {
          d[w++] = (uint8_t)(moff & 0xff);
          d[w++] = (uint8_t)(moff >> 8);
          if (ml_token >= 15) {
            int32_t r = ml_token - 15;
            while (r >= 255) { d[w++] = 255; r -= 255; }
            d[w++] = (uint8_t)r;
          }
        }
      };
      if (blen >= 13) {
        int32_t misses = 0;  // LZ4-style skip acceleration: after a run of
        while (pos <= mflimit && !overflow) {  // misses, stride grows so
          uint32_t v;                          // incompressible data is
          __builtin_memcpy(&v, s + pos, 4);    // skimmed, not crawled
          const uint32_t h = (v * 2654435761u) >> (32 - LZ4_HASH_LOG);
          const int32_t cand = tab[h] == 0xffff ? -1 : (int32_t)tab[h];
          tab[h] = (uint16_t)pos;
          uint32_t cv = 0;
          if (cand >= 0) __builtin_memcpy(&cv, s + cand, 4);
          if (cand >= 0 && cv == v) {
            int32_t mlen = 4;
            while (pos + mlen < matchlimit && s[cand + mlen] == s[pos + mlen])
              ++mlen;
            emit_seq(pos - anchor, mlen, pos - cand);
            pos += mlen;
            anchor = pos;
            misses = 0;
          } else {
            pos += 1 + (misses >> 6);
            ++misses;
          }
        }
      }
      // trailing literals-only sequence
      if (!overflow) emit_seq(blen - anchor, -1, 0);
      result = (overflow || w >= blen) ? -(int64_t)blen : (int64_t)w;
    }
    result = bcast64(result);
    // stored blocks: the whole wave copies raw bytes into the slot
    if (result < 0)
      for (int32_t i = lane; i < blen; i += BG_WAVE) d[i] = s[i];
  }
  return result;
}

__global__ void k_lz4_compress(const uint8_t* src, int64_t len,
                               uint8_t* out_slots, int64_t slot_stride,
                               int64_t* block_sizes, int64_t nblocks) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  uint16_t* tab_all = reinterpret_cast<uint16_t*>(smem_raw);
  const int wave_in_block = threadIdx.x / BG_WAVE;
  uint16_t* tab = tab_all + (size_t)wave_in_block * (1 << LZ4_HASH_LOG);
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t b = wave_global; b < nblocks; b += nwaves) {
    const int64_t boff = b * BG_LZ4_BLOCK;
    const int32_t blen = (int32_t)(len - boff < BG_LZ4_BLOCK ? len - boff
                                                          : BG_LZ4_BLOCK);
    const int64_t r = lz4_compress_one(src + boff, blen,
                                       out_slots + b * slot_stride, tab);
    if (lane_id() == 0) block_sizes[b] = r;
  }
}

// flat batched form: one wave per (buffer, block) pair across many buffers
__global__ void k_lz4_compress_flat(const bg_lz4_block_job* jobs, int64_t njobs,
                                    int64_t* block_sizes) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  uint16_t* tab_all = reinterpret_cast<uint16_t*>(smem_raw);
  const int wave_in_block = threadIdx.x / BG_WAVE;
  uint16_t* tab = tab_all + (size_t)wave_in_block * (1 << LZ4_HASH_LOG);
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t j = wave_global; j < njobs; j += nwaves) {
    const bg_lz4_block_job job = jobs[j];
    const int64_t r =
        lz4_compress_one(job.d_src, job.blen, job.d_dst_slot, tab);
    if (lane_id() == 0) block_sizes[j] = r;
  }
}

extern "C" int bg_lz4_compress_flat(const bg_lz4_block_job* h_jobs,
                                    int64_t njobs, int64_t* h_block_sizes) {
  REQUIRE_INIT();
  DevBuf<bg_lz4_block_job> d_jobs;
  DevBuf<int64_t> d_sizes;
  HIP_TRY(d_jobs.alloc(njobs));
  HIP_TRY(d_sizes.alloc(njobs));
  HIP_TRY(hipMemcpy(d_jobs, h_jobs, sizeof(bg_lz4_block_job) * njobs,
                    hipMemcpyHostToDevice));
  const int waves_per_block = BG_BLOCK / BG_WAVE;
  const size_t lds = (size_t)waves_per_block * (1 << LZ4_HASH_LOG) *
                     sizeof(uint16_t);
  int blocks = grid_for(njobs, waves_per_block);
  hipLaunchKernelGGL(k_lz4_compress_flat, dim3(blocks), dim3(BG_BLOCK), lds, 0,
                     d_jobs, njobs, d_sizes);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(h_block_sizes, d_sizes, sizeof(int64_t) * njobs,
                    hipMemcpyDeviceToHost));
  return BG_OK;
}

extern "C" int bg_lz4_compress(const void* d_src, int64_t len,
                               void* d_out_slots, int64_t* h_block_sizes,
                               int64_t* out_nblocks) {
  REQUIRE_INIT();
  const int64_t nblocks = (len + BG_LZ4_BLOCK - 1) / BG_LZ4_BLOCK;
  DevBuf<int64_t> d_sizes;
  HIP_TRY(d_sizes.alloc(nblocks));
  const int waves_per_block = BG_BLOCK / BG_WAVE;
  const size_t lds = (size_t)waves_per_block * (1 << LZ4_HASH_LOG) *
                     sizeof(uint16_t);
  int blocks = grid_for(nblocks, waves_per_block);
  hipLaunchKernelGGL(k_lz4_compress, dim3(blocks), dim3(BG_BLOCK), lds, 0,
                     (const uint8_t*)d_src, len, (uint8_t*)d_out_slots,
                     (int64_t)BG_LZ4_SLOT_STRIDE, d_sizes, nblocks);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(h_block_sizes, d_sizes, sizeof(int64_t) * nblocks,
                    hipMemcpyDeviceToHost));
  *out_nblocks = nblocks;
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Batched block pack: assemble LZ4 frame bodies on device — each job writes
// its [u32 size-word][block bytes] at the precomputed frame offset, so the
// host downloads ONE contiguous compressed stream per buffer (no
// slot-strided D2H, no host-side slicing).
// ---------------------------------------------------------------------------
__global__ void k_pack_blocks(const bg_pack_job* jobs, int64_t njobs) {
  for (int64_t j = blockIdx.x; j < njobs; j += gridDim.x) {
    const bg_pack_job job = jobs[j];
    if (threadIdx.x == 0) {
      job.d_dst[0] = (uint8_t)(job.size_word & 0xff);
      job.d_dst[1] = (uint8_t)((job.size_word >> 8) & 0xff);
      job.d_dst[2] = (uint8_t)((job.size_word >> 16) & 0xff);
      job.d_dst[3] = (uint8_t)((job.size_word >> 24) & 0xff);
    }
    uint8_t* d = job.d_dst + 4;
    for (int64_t i = threadIdx.x; i < job.nbytes; i += blockDim.x)
      d[i] = job.d_src[i];
  }
}

extern "C" int bg_pack_blocks(const bg_pack_job* h_jobs, int64_t njobs) {
  REQUIRE_INIT();
  DevBuf<bg_pack_job> d_jobs;
  HIP_TRY(d_jobs.alloc(njobs));
  HIP_TRY(hipMemcpy(d_jobs, h_jobs, sizeof(bg_pack_job) * njobs,
                    hipMemcpyHostToDevice));
  int blocks = grid_for(njobs, 1);
  hipLaunchKernelGGL(k_pack_blocks, dim3(blocks), dim3(BG_BLOCK), 0, 0, d_jobs,
                     njobs);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Fused hash-repartition materialiser (k <= 64, <= 4 fixed-width payload
// columns): ONE pass recomputes the key hash (cheaper than writing/reading
// a pids array), ranks rows per partition with ballots, stages rows in
// per-partition LDS tiles and flushes 64-row bursts per column — write
// combining turns the k scattered payload streams into contiguous
// wave-wide stores.  Start offsets come from the same hist+scan prework
// as the stable split (chunk-contiguous => stable order preserved).
// ---------------------------------------------------------------------------
#define FM_TILE 64
#define FM_WAVES 2  // waves per 128-thread block (LDS budget)

struct FmArgs {
  KeyArgs keys;
  int ncols;
  struct {
    const void* data;
    void* out;
    int esz;  // 1/4/8/16
  } c[BG_MAX_KEYS];
};

__global__ void __launch_bounds__(FM_WAVES * BG_WAVE)
k_fused_materialize(FmArgs args, int64_t n, uint32_t k, const i64* start,
                    int64_t nchunks, uint32_t* out_idx, uint32_t* rank_out) {
  // LDS: per wave: [k][FM_TILE] u32 row-index tile + per-col value tiles
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int wave_in_block = threadIdx.x / BG_WAVE;
  const int lane = lane_id();
  // layout per wave: idx tile (k*FM_TILE*4) + cols (k*FM_TILE*esz each)
  size_t wave_bytes = (size_t)k * FM_TILE * 4;
  for (int c = 0; c < args.ncols; ++c)
    wave_bytes += (size_t)k * FM_TILE * args.c[c].esz;
  char* base = smem_raw + (size_t)wave_in_block * wave_bytes;
  uint32_t* t_idx = reinterpret_cast<uint32_t*>(base);
  char* t_cols[BG_MAX_KEYS];
  {
    char* p = base + (size_t)k * FM_TILE * 4;
    for (int c = 0; c < args.ncols; ++c) {
      t_cols[c] = p;
      p += (size_t)k * FM_TILE * args.c[c].esz;
    }
  }
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t ch = wave_global; ch < nchunks; ch += nwaves) {
    // register cursors: lane p holds partition p's next global slot and
    // the count of rows THIS WAVE has staged-but-not-flushed (cursors are
    // not tile-aligned: tile slot 0 sits at global position cursor - fill)
    i64 my_cursor = (lane < (int)k)
                        ? start[(int64_t)lane * nchunks + ch]
                        : 0;
    int my_fill = 0;
    const int64_t r0 = ch * PS_ROWS_PER_WAVE;
    const int64_t r1 = min(r0 + (int64_t)PS_ROWS_PER_WAVE, n);
    for (int64_t rb = r0; rb < r1; rb += BG_WAVE) {
      const int64_t r = rb + lane;
      const bool active = r < r1;
      uint32_t pid = 0xffffffffu;
      if (active) {
        const u64 h = hash_keys_row(args.keys, r);
        pid = (uint32_t)(h % (u64)k);
      }
      for (uint32_t p = 0; p < k; ++p) {
        const u64 m = __ballot(active && pid == p);
        if (!m) continue;
        const i64 cur =
            ((i64)(uint32_t)__builtin_amdgcn_readlane(
                 (int)(uint32_t)((u64)my_cursor >> 32), p)
             << 32) |
            (i64)(uint32_t)__builtin_amdgcn_readlane(
                (int)(uint32_t)((u64)my_cursor & 0xffffffff), p);
        const int fill = __builtin_amdgcn_readlane(my_fill, p);
        const int cnt = __popcll(m);
        const int rank = __popcll(m & ((1ull << lane) - 1));
        const int slot = fill + rank;
        const bool mine = active && pid == p;
        if (mine && slot < FM_TILE) {
          t_idx[p * FM_TILE + slot] = (uint32_t)r;
          for (int c = 0; c < args.ncols; ++c) {
            switch (args.c[c].esz) {
              case 1:
                t_cols[c][p * FM_TILE + slot] =
                    reinterpret_cast<const uint8_t*>(args.c[c].data)[r];
                break;
              case 4:
                reinterpret_cast<uint32_t*>(t_cols[c])[p * FM_TILE + slot] =
                    reinterpret_cast<const uint32_t*>(args.c[c].data)[r];
                break;
              case 8:
                reinterpret_cast<u64*>(t_cols[c])[p * FM_TILE + slot] =
                    reinterpret_cast<const u64*>(args.c[c].data)[r];
                break;
              case 16:
                reinterpret_cast<ulong2*>(t_cols[c])[p * FM_TILE + slot] =
                    reinterpret_cast<const ulong2*>(args.c[c].data)[r];
                break;
            }
          }
        }
        if (mine && rank_out) rank_out[r] = (uint32_t)(cur + rank);
        __builtin_amdgcn_wave_barrier();
        // tile crossed a 64 boundary? flush the completed tile
        const int new_fill = fill + cnt;
        if (new_fill >= FM_TILE) {
          const i64 flush_base = cur - fill;  // global position of slot 0
          for (int i = lane; i < FM_TILE; i += BG_WAVE)
            out_idx[flush_base + i] = t_idx[p * FM_TILE + i];
          for (int c = 0; c < args.ncols; ++c) {
            switch (args.c[c].esz) {
              case 1:
                for (int i = lane; i < FM_TILE; i += BG_WAVE)
                  reinterpret_cast<uint8_t*>(args.c[c].out)[flush_base + i] =
                      t_cols[c][p * FM_TILE + i];
                break;
              case 4:
                for (int i = lane; i < FM_TILE; i += BG_WAVE)
                  reinterpret_cast<uint32_t*>(args.c[c].out)[flush_base + i] =
                      reinterpret_cast<uint32_t*>(t_cols[c])[p * FM_TILE + i];
                break;
              case 8:
                for (int i = lane; i < FM_TILE; i += BG_WAVE)
                  reinterpret_cast<u64*>(args.c[c].out)[flush_base + i] =
                      reinterpret_cast<u64*>(t_cols[c])[p * FM_TILE + i];
                break;
              case 16:
                for (int i = lane; i < FM_TILE; i += BG_WAVE)
                  reinterpret_cast<ulong2*>(args.c[c].out)[flush_base + i] =
                      reinterpret_cast<ulong2*>(t_cols[c])[p * FM_TILE + i];
                break;
            }
          }
          __builtin_amdgcn_wave_barrier();
          // restage this group's overflow rows into the emptied tile
          if (mine && slot >= FM_TILE) {
            const int slot2 = slot - FM_TILE;
            t_idx[p * FM_TILE + slot2] = (uint32_t)r;
            for (int c = 0; c < args.ncols; ++c) {
              switch (args.c[c].esz) {
                case 1:
                  t_cols[c][p * FM_TILE + slot2] =
                      reinterpret_cast<const uint8_t*>(args.c[c].data)[r];
                  break;
                case 4:
                  reinterpret_cast<uint32_t*>(t_cols[c])[p * FM_TILE + slot2] =
                      reinterpret_cast<const uint32_t*>(args.c[c].data)[r];
                  break;
                case 8:
                  reinterpret_cast<u64*>(t_cols[c])[p * FM_TILE + slot2] =
                      reinterpret_cast<const u64*>(args.c[c].data)[r];
                  break;
                case 16:
                  reinterpret_cast<ulong2*>(t_cols[c])[p * FM_TILE + slot2] =
                      reinterpret_cast<const ulong2*>(args.c[c].data)[r];
                  break;
              }
            }
          }
        }
        // cursor/fill advance on owning lane
        if (lane == (int)p) {
          my_cursor += cnt;
          my_fill = new_fill >= FM_TILE ? new_fill - FM_TILE : new_fill;
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
    // chunk done: flush partial tiles (fill rows each)
    for (uint32_t p = 0; p < k; ++p) {
      const i64 cur =
          ((i64)(uint32_t)__builtin_amdgcn_readlane(
               (int)(uint32_t)((u64)my_cursor >> 32), p)
           << 32) |
          (i64)(uint32_t)__builtin_amdgcn_readlane(
              (int)(uint32_t)((u64)my_cursor & 0xffffffff), p);
      const int fill = __builtin_amdgcn_readlane(my_fill, p);
      if (!fill) continue;
      const i64 flush_base = cur - fill;
      // tile slots [0, fill) hold this wave's staged rows for positions
      // [flush_base, cur); flush them
      for (int i = lane; i < fill; i += BG_WAVE)
        out_idx[flush_base + i] = t_idx[p * FM_TILE + i];
      for (int c = 0; c < args.ncols; ++c) {
        switch (args.c[c].esz) {
          case 1:
            for (int i = lane; i < fill; i += BG_WAVE)
              reinterpret_cast<uint8_t*>(args.c[c].out)[flush_base + i] =
                  t_cols[c][p * FM_TILE + i];
            break;
          case 4:
            for (int i = lane; i < fill; i += BG_WAVE)
              reinterpret_cast<uint32_t*>(args.c[c].out)[flush_base + i] =
                  reinterpret_cast<uint32_t*>(t_cols[c])[p * FM_TILE + i];
            break;
          case 8:
            for (int i = lane; i < fill; i += BG_WAVE)
              reinterpret_cast<u64*>(args.c[c].out)[flush_base + i] =
                  reinterpret_cast<u64*>(t_cols[c])[p * FM_TILE + i];
            break;
          case 16:
            for (int i = lane; i < fill; i += BG_WAVE)
              reinterpret_cast<ulong2*>(args.c[c].out)[flush_base + i] =
                  reinterpret_cast<ulong2*>(t_cols[c])[p * FM_TILE + i];
            break;
        }
      }
    }
  }
}

extern "C" int bg_hash_repartition_fused(const bg_column* key_cols,
                                         int32_t nkeys,
                                         const bg_column* payload_cols,
                                         int32_t ncols, int64_t n, uint32_t k,
                                         uint32_t* d_indices,
                                         int64_t* d_offsets, uint32_t* d_rank,
                                         void** d_out) {
  REQUIRE_INIT();
  if (k == 0 || k > BG_WAVE)
    return set_err(BG_ERR_INVALID, "fused path needs k in [1,64]");
  if (ncols > BG_MAX_KEYS)
    return set_err(BG_ERR_INVALID, "fused path: <= 4 payload cols");
  KeyArgs keys{};
  keys.nkeys = nkeys;
  for (int i = 0; i < nkeys; ++i) {
    keys.k[i].data = key_cols[i].d_data;
    keys.k[i].valid = key_cols[i].d_validity;
    keys.k[i].offsets = key_cols[i].d_offsets;
    keys.k[i].dtype = key_cols[i].dtype;
  }
  FmArgs a{};
  a.keys = keys;
  a.ncols = ncols;
  size_t wave_bytes = (size_t)k * FM_TILE * 4;
  for (int i = 0; i < ncols; ++i) {
    a.c[i].data = payload_cols[i].d_data;
    a.c[i].out = d_out[i];
    int esz = (int)dtype_size(payload_cols[i].dtype);
    if (esz != 1 && esz != 4 && esz != 8 && esz != 16)
      return set_err(BG_ERR_UNSUPPORTED, "fused payload dtype");
    a.c[i].esz = esz;
    wave_bytes += (size_t)k * FM_TILE * esz;
  }
  const size_t lds = wave_bytes * FM_WAVES;
  if (lds > 160 * 1024)
    return set_err(BG_ERR_INVALID, "fused path LDS budget exceeded");

  // hist + scan prework (same stability contract as the split)
  const int64_t nchunks = (n + PS_ROWS_PER_WAVE - 1) / PS_ROWS_PER_WAVE;
  const int64_t hist_len = (int64_t)k * (nchunks ? nchunks : 1);
  DevBuf<uint32_t> d_pids;
  DevBuf<u64> d_hist;
  DevBuf<i64> d_start;
  HIP_TRY(d_pids.alloc(n));
  HIP_TRY(d_hist.alloc(hist_len));
  HIP_TRY(d_start.alloc(hist_len));
  DevBuf<uint64_t> d_hashes;
  HIP_TRY(d_hashes.alloc(n));
  int rc = bg_hash_columns(key_cols, nkeys, n, d_hashes);
  if (rc == BG_OK) rc = bg_partition_ids(d_hashes, n, k, d_pids);
  d_hashes.reset();  // n-sized: back to the pool before the scan allocates
  if (rc == BG_OK) {
    const int waves_per_block = BG_BLOCK / BG_WAVE;
    const size_t lds_hist = (size_t)waves_per_block * k * sizeof(uint32_t);
    int blocks = grid_for(nchunks, 1);
    hipLaunchKernelGGL(k_part_hist, dim3(blocks), dim3(BG_BLOCK), lds_hist, 0,
                       d_pids, n, k, d_hist, nchunks);
    rc = scan_exclusive_i64(d_hist, hist_len, d_start, nullptr);
  }
  if (rc == BG_OK) {
    hipLaunchKernelGGL(k_extract_offsets, dim3(1), dim3(BG_BLOCK), 0, 0,
                       d_start, nchunks, k, n, d_offsets);
    const int64_t fm_threads = FM_WAVES * BG_WAVE;
    int blocks = grid_for(nchunks, 1);
    EventPair ev;
    (void)ev.create();
    (void)hipEventRecord(ev.ev0, 0);
    hipLaunchKernelGGL(k_fused_materialize, dim3(blocks), dim3(fm_threads),
                       lds, 0, a, n, k, d_start, nchunks, d_indices, d_rank);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = set_hip_err(e, "fused materialize");
    (void)hipEventRecord(ev.ev1, 0);
    (void)hipEventSynchronize(ev.ev1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.ev0, ev.ev1);
    g_last_kernel_ms = (double)ms;
  }
  return rc;
}

// ---------------------------------------------------------------------------
// LZ4-frame DECODE (device shuffle-read ingest — the decompress mirror of
// bg_lz4_compress, so a GPU-resident next stage can consume shuffle bytes
// without host decode).  One wave per frame: lane 0 parses the frame
// header and each block's size word + the LZ4 sequences; 64 lanes execute
// literal/match copies (pattern replication via modulo, as in Snappy).
// Handles stored blocks (high-bit size) and linked or independent blocks
// (the output is contiguous, so back-references past block starts work).
// ---------------------------------------------------------------------------
__global__ void k_lz4_decompress(const bg_lz4_frame* frames, int64_t nframes,
                                 int64_t* out_lens) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  const int lane = lane_id();
  for (int64_t f = wave_global; f < nframes; f += nwaves) {
    const uint8_t* s = frames[f].d_src;
    const uint8_t* send = s + frames[f].src_len;
    uint8_t* base_d = frames[f].d_dst;
    const int64_t dcap = frames[f].dst_cap;
    int ok = 1;
    int64_t si = 0, di = 0;
    if (lane == 0) {
      // magic + FLG/BD/HC; flags: content-size bit adds 8 bytes, dict-id 4
      if (si + 7 > frames[f].src_len ||
          s[0] != 0x04 || s[1] != 0x22 || s[2] != 0x4d || s[3] != 0x18) {
        ok = 0;
      } else {
        const uint8_t flg = s[4];
        si = 7;
        if (flg & 0x08) si += 8;  // content size
        if (flg & 0x01) si += 4;  // dict id
        if (flg & 0x10) ok = 0;   // block checksums unsupported
      }
    }
    ok = bcast32(ok);
    si = bcast64(si);
    while (ok) {
      // lane 0 reads the block size word
      int64_t bsize = 0;
      int stored = 0;
      if (lane == 0) {
        if (si + 4 > frames[f].src_len) { ok = 0; }
        else {
          uint32_t w = (uint32_t)s[si] | ((uint32_t)s[si + 1] << 8) |
                       ((uint32_t)s[si + 2] << 16) |
                       ((uint32_t)s[si + 3] << 24);
          si += 4;
          if (w == 0) { bsize = -1; }  // end mark
          else {
            stored = (w >> 31) & 1;
            bsize = (int64_t)(w & 0x7fffffff);
          }
        }
      }
      ok = bcast32(ok);
      if (!ok) break;
      bsize = bcast64(bsize);
      stored = bcast32(stored);
      si = bcast64(si);
      if (bsize < 0) break;  // end mark
      if (stored) {
        if (lane == 0 && (si + bsize > frames[f].src_len ||
                          di + bsize > dcap))
          ok = 0;
        ok = bcast32(ok);
        if (!ok) break;
        for (int64_t i = lane; i < bsize; i += BG_WAVE)
          base_d[di + i] = s[si + i];
        si += bsize;
        di += bsize;
        continue;
      }
      // LZ4 block: sequences until block exhausted
      const int64_t bend = si + bsize;
      while (ok && si < bend) {
        // lane 0 parses one full sequence: token, literal length (+ext),
        // literal start, optional match offset + length (+ext)
        int64_t lit_len = 0, mlen = 0, moff = 0, lsrc = 0, nsi = si;
        if (lane == 0) {
          const uint8_t token = s[nsi++];
          lit_len = token >> 4;
          if (lit_len == 15) {
            while (nsi < bend) {
              const uint8_t b = s[nsi++];
              lit_len += b;
              if (b != 255) break;
            }
          }
          lsrc = nsi;
          nsi += lit_len;
          if (nsi > bend || di + lit_len > dcap) {
            ok = 0;
          } else if (nsi < bend) {  // a match follows
            if (nsi + 2 > bend) {
              ok = 0;
            } else {
              moff = (int64_t)s[nsi] | ((int64_t)s[nsi + 1] << 8);
              nsi += 2;
              mlen = token & 0x0f;
              if (mlen == 15) {
                while (nsi < bend) {
                  const uint8_t b = s[nsi++];
                  mlen += b;
                  if (b != 255) break;
                }
              }
              mlen += 4;
              if (moff == 0 || moff > di + lit_len ||
                  di + lit_len + mlen > dcap)
                ok = 0;
            }
          }
        }
        ok = bcast32(ok);
        if (!ok) break;
        lit_len = bcast64(lit_len);
        mlen = bcast64(mlen);
        moff = bcast64(moff);
        lsrc = bcast64(lsrc);
        nsi = bcast64(nsi);
        for (int64_t i = lane; i < lit_len; i += BG_WAVE)
          base_d[di + i] = s[lsrc + i];
        di += lit_len;
        if (mlen) {
          const uint8_t* win = base_d + di - moff;
          uint8_t* dst = base_d + di;
          if (moff >= mlen) {
            for (int64_t i = lane; i < mlen; i += BG_WAVE) dst[i] = win[i];
          } else {
            for (int64_t i = lane; i < mlen; i += BG_WAVE)
              dst[i] = win[i % moff];
          }
          di += mlen;
        }
        si = nsi;
      }
    }
    if (lane == 0) out_lens[f] = ok ? di : -1;
  }
}

extern "C" int bg_lz4_decompress(const bg_lz4_frame* h_frames, int64_t nframes,
                                 int64_t* h_out_lens) {
  REQUIRE_INIT();
  DevBuf<bg_lz4_frame> d_frames;
  DevBuf<int64_t> d_lens;
  HIP_TRY(d_frames.alloc(nframes));
  HIP_TRY(d_lens.alloc(nframes));
  HIP_TRY(hipMemcpy(d_frames, h_frames, sizeof(bg_lz4_frame) * nframes,
                    hipMemcpyHostToDevice));
  const int waves_per_block = BG_BLOCK / BG_WAVE;
  int blocks = grid_for(nframes, waves_per_block);
  hipLaunchKernelGGL(k_lz4_decompress, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     d_frames, nframes, d_lens);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(h_out_lens, d_lens, sizeof(int64_t) * nframes,
                    hipMemcpyDeviceToHost));
  return BG_OK;
}

// ---------------------------------------------------------------------------
// stage-interpreter support kernels (bg_execute_stage, stage.cpp):
//  - bg_set_error: lets the separate stage.cpp translation unit report
//    through the same thread-local bg_last_error channel
//  - bg_bitcopy: place a batch's decompressed Arrow validity bits into a
//    column bitmap at an arbitrary bit offset (device shuffle read crosses
//    batch boundaries that are not byte-aligned)
//  - bg_agg_materialize / bg_avg_finalize: turn bg_hashagg accumulator
//    records into Arrow output columns on device (the final/single
//    AggregateExec materialisation, incl. SQL all-NULL-group semantics and
//    DataFusion's decimal AVG scale rules)
// ---------------------------------------------------------------------------

extern "C" int bg_set_error(int code, const char* msg) {
  return set_err(code, msg);
}

__global__ void k_bitcopy(const uint8_t* __restrict__ src, int64_t nbits,
                          uint32_t* __restrict__ dst, int64_t dst_bit_off) {
  // each thread owns one 32-bit destination word of the target range;
  // boundary words shared with neighbouring batches go through atomics
  const int64_t w0 = dst_bit_off >> 5;
  const int64_t w1 = (dst_bit_off + nbits - 1) >> 5;
  for (int64_t w = w0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       w <= w1; w += (int64_t)gridDim.x * blockDim.x) {
    uint32_t value = 0, mask = 0;
    const int64_t base_bit = (w << 5);
    for (int b = 0; b < 32; ++b) {
      const int64_t src_bit = base_bit + b - dst_bit_off;
      if (src_bit < 0 || src_bit >= nbits) continue;
      mask |= (1u << b);
      if ((src[src_bit >> 3] >> (src_bit & 7)) & 1) value |= (1u << b);
    }
    if (mask == 0xffffffffu) {
      dst[w] = value;
    } else {
      atomicAnd(&dst[w], ~mask);
      atomicOr(&dst[w], value);
    }
  }
}

extern "C" int bg_bitcopy(const uint8_t* d_src_bits, int64_t nbits,
                          uint8_t* d_dst_bits, int64_t dst_bit_off) {
  REQUIRE_INIT();
  if (nbits <= 0) return BG_OK;
  int64_t words = ((dst_bit_off + nbits) >> 5) - (dst_bit_off >> 5) + 1;
  int blocks = grid_for(words);
  hipLaunchKernelGGL(k_bitcopy, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     d_src_bits, nbits, (uint32_t*)d_dst_bits, dst_bit_off);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// accumulator -> natural value transforms (inverse of the kernels' order-
// preserving encodings; mirrors gpu.py decode_agg_value)
__global__ void k_agg_materialize(const uint8_t* __restrict__ acc,
                                  int64_t acc_stride, int32_t op,
                                  int64_t ngroups, uint8_t* __restrict__ out,
                                  const int64_t* __restrict__ nncnt,
                                  int64_t nncnt_stride,
                                  uint32_t* __restrict__ valid_out) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups;
       g += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t* a = acc + g * acc_stride;
    const uint64_t lo = *reinterpret_cast<const uint64_t*>(a);
    const uint64_t hi = *reinterpret_cast<const uint64_t*>(a + 8);
    bool is_null = false;
    if (nncnt) {
      const int64_t nn = *reinterpret_cast<const int64_t*>(
          reinterpret_cast<const uint8_t*>(nncnt) + g * nncnt_stride);
      is_null = (nn == 0);
      if (valid_out) {
        if (is_null) atomicAnd(&valid_out[g >> 5], ~(1u << (g & 31)));
        else atomicOr(&valid_out[g >> 5], 1u << (g & 31));
      }
    }
    switch (op) {
      case BG_AGG_OP_SUM_DEC128: {  // i128 LE, 16-B out
        uint64_t* o = reinterpret_cast<uint64_t*>(out + g * 16);
        o[0] = is_null ? 0 : lo;
        o[1] = is_null ? 0 : hi;
        break;
      }
      case BG_AGG_OP_SUM_I64: {  // low limb as i64
        reinterpret_cast<int64_t*>(out)[g] = is_null ? 0 : (int64_t)lo;
        break;
      }
      case BG_AGG_OP_SUM_F64: {
        reinterpret_cast<uint64_t*>(out)[g] = is_null ? 0 : lo;
        break;
      }
      case BG_AGG_OP_MAX_I64: {
        reinterpret_cast<int64_t*>(out)[g] =
            is_null ? 0 : (int64_t)(lo ^ 0x8000000000000000ull);
        break;
      }
      case BG_AGG_OP_MIN_I64: {
        reinterpret_cast<int64_t*>(out)[g] =
            is_null ? 0 : (int64_t)((~lo) ^ 0x8000000000000000ull);
        break;
      }
      case BG_AGG_OP_MIN_F64:
      case BG_AGG_OP_MAX_F64: {
        uint64_t enc = lo;
        if (op == BG_AGG_OP_MIN_F64) enc = ~enc;
        uint64_t bits = (enc >> 63) ? (enc ^ 0x8000000000000000ull) : ~enc;
        reinterpret_cast<uint64_t*>(out)[g] = is_null ? 0 : bits;
        break;
      }
      case BG_AGG_OP_MAX_I32: {  // 4-B out (Int32/Date32)
        reinterpret_cast<int32_t*>(out)[g] =
            is_null ? 0 : (int32_t)(int64_t)(lo ^ 0x8000000000000000ull);
        break;
      }
      case BG_AGG_OP_MIN_I32: {
        reinterpret_cast<int32_t*>(out)[g] =
            is_null ? 0 : (int32_t)(int64_t)((~lo) ^ 0x8000000000000000ull);
        break;
      }
      default: break;
    }
  }
}

extern "C" int bg_agg_materialize(const void* d_acc, int64_t acc_stride,
                                  int32_t op, int64_t ngroups, void* d_out,
                                  const int64_t* d_nncnt,
                                  int64_t nncnt_stride,
                                  uint8_t* d_valid_out) {
  REQUIRE_INIT();
  if (op == BG_AGG_OP_MIN_ROW || op == BG_AGG_OP_MAX_ROW)
    // the record names a row of an input column this call never sees
    return set_err(BG_ERR_INVALID,
                   "bg_agg_materialize: MIN_ROW/MAX_ROW hold a row index "
                   "(bg_agg_winner_rows + bg_gather)");
  if (ngroups <= 0) return BG_OK;
  int blocks =
      (int)bg_imin64((ngroups + BG_BLOCK - 1) / BG_BLOCK, BG_MAX_BLOCKS);
  hipLaunchKernelGGL(k_agg_materialize, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (const uint8_t*)d_acc, acc_stride, op, ngroups,
                     (uint8_t*)d_out, d_nncnt, nncnt_stride,
                     (uint32_t*)d_valid_out);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// MIN_ROW/MAX_ROW records -> gather indices + validity.  One thread owns
// one whole byte of the bitmap (8 groups), so it needs no atomics and no
// pre-initialised bitmap; bits past ngroups in the last byte are 0.
__global__ void k_agg_winner_rows(const uint8_t* __restrict__ acc,
                                  int64_t acc_stride, int64_t ngroups,
                                  uint32_t* __restrict__ rows_out,
                                  uint8_t* __restrict__ valid_out) {
  const int64_t nbytes = (ngroups + 7) / 8;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nbytes;
       b += (int64_t)gridDim.x * blockDim.x) {
    uint8_t bits = 0;
    for (int j = 0; j < 8; ++j) {
      const int64_t g = b * 8 + j;
      if (g >= ngroups) break;
      const uint64_t w =
          *reinterpret_cast<const uint64_t*>(acc + g * acc_stride);
      rows_out[g] = w ? (uint32_t)(w - 1) : 0u;
      if (w) bits |= (uint8_t)(1u << j);
    }
    valid_out[b] = bits;
  }
}

extern "C" int bg_agg_winner_rows(const void* d_acc, int64_t acc_stride,
                                  int64_t ngroups, uint32_t* d_rows_out,
                                  uint8_t* d_valid_out) {
  REQUIRE_INIT();
  if (ngroups <= 0) return BG_OK;
  const int64_t nbytes = (ngroups + 7) / 8;
  int blocks =
      (int)bg_imin64((nbytes + BG_BLOCK - 1) / BG_BLOCK, BG_MAX_BLOCKS);
  hipLaunchKernelGGL(k_agg_winner_rows, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (const uint8_t*)d_acc, acc_stride, ngroups, d_rows_out,
                     d_valid_out);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// strided i64 copy (COUNT / non-null-count materialisation)
__global__ void k_copy_i64_strided(const uint8_t* __restrict__ src,
                                   int64_t stride, int64_t n,
                                   int64_t* __restrict__ out) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n;
       g += (int64_t)gridDim.x * blockDim.x)
    out[g] = *reinterpret_cast<const int64_t*>(src + g * stride);
}

extern "C" int bg_copy_i64_strided(const void* d_src, int64_t stride,
                                   int64_t n, void* d_out) {
  REQUIRE_INIT();
  if (n <= 0) return BG_OK;
  int blocks = (int)bg_imin64((n + BG_BLOCK - 1) / BG_BLOCK, BG_MAX_BLOCKS);
  hipLaunchKernelGGL(k_copy_i64_strided, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (const uint8_t*)d_src, stride, n, (int64_t*)d_out);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// AVG finalisation.  Decimal: DataFusion's AvgAccumulator for Decimal128
// (datafusion/functions-aggregate avg.rs): target scale = input scale + 4,
// value = round_half_up(sum * 10^4 / count) computed exactly in i128.
// Float64: IEEE division.  d_cnt entries of 0 yield NULL (valid bit clear).
__global__ void k_avg_finalize(const uint8_t* __restrict__ acc,
                               int64_t acc_stride, int32_t is_f64,
                               const uint8_t* __restrict__ cnt,
                               int64_t cnt_stride, int32_t scale_shift,
                               int64_t ngroups, uint8_t* __restrict__ out,
                               uint32_t* __restrict__ valid_out) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups;
       g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = *reinterpret_cast<const int64_t*>(cnt + g * cnt_stride);
    if (valid_out) {
      if (c == 0) atomicAnd(&valid_out[g >> 5], ~(1u << (g & 31)));
      else atomicOr(&valid_out[g >> 5], 1u << (g & 31));
    }
    if (is_f64) {
      const double s =
          *reinterpret_cast<const double*>(acc + g * acc_stride);
      reinterpret_cast<double*>(out)[g] = c ? s / (double)c : 0.0;
      continue;
    }
    __int128 s = (__int128)(
        ((unsigned __int128)*reinterpret_cast<const uint64_t*>(
             acc + g * acc_stride + 8)
         << 64) |
        *reinterpret_cast<const uint64_t*>(acc + g * acc_stride));
    __int128 v = 0;
    if (c) {
      __int128 p10 = 1;
      for (int i = 0; i < scale_shift; ++i) p10 *= 10;
      __int128 num = s * p10;
      const bool neg = num < 0;
      unsigned __int128 un = neg ? (unsigned __int128)(-num)
                                 : (unsigned __int128)num;
      const unsigned __int128 uc = (unsigned __int128)c;
      unsigned __int128 q = un / uc;
      const unsigned __int128 r = un - q * uc;
      if (2 * r >= uc) q += 1;  // round half away from zero
      v = neg ? -(__int128)q : (__int128)q;
    }
    uint64_t* o = reinterpret_cast<uint64_t*>(out + g * 16);
    o[0] = (uint64_t)v;
    o[1] = (uint64_t)(v >> 64);
  }
}

extern "C" int bg_avg_finalize(const void* d_sum_acc, int64_t acc_stride,
                               int32_t is_f64, const void* d_cnt,
                               int64_t cnt_stride, int32_t scale_shift,
                               int64_t ngroups, void* d_out,
                               uint8_t* d_valid_out) {
  REQUIRE_INIT();
  if (ngroups <= 0) return BG_OK;
  int blocks =
      (int)bg_imin64((ngroups + BG_BLOCK - 1) / BG_BLOCK, BG_MAX_BLOCKS);
  hipLaunchKernelGGL(k_avg_finalize, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (const uint8_t*)d_sum_acc, acc_stride, is_f64,
                     (const uint8_t*)d_cnt, cnt_stride, scale_shift, ngroups,
                     (uint8_t*)d_out, (uint32_t*)d_valid_out);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// synthetic-data fill for the no-Python C++ examples/bench (splitmix64
// per element — deterministic, seed+index addressed; TEST/BENCH
// INFRASTRUCTURE, not on any query path)
__global__ void k_fill_rand(uint8_t* __restrict__ out, int64_t n,
                            uint64_t seed, int64_t lo, uint64_t range,
                            int32_t mode) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t z = seed + (uint64_t)i * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    int64_t v = lo + (int64_t)(z % range);
    switch (mode) {
      case 0: reinterpret_cast<int64_t*>(out)[i] = v; break;
      case 1: reinterpret_cast<int32_t*>(out)[i] = (int32_t)v; break;
      case 2: {  // Decimal128 LE pair
        int64_t* p = reinterpret_cast<int64_t*>(out) + 2 * i;
        p[0] = v;
        p[1] = v < 0 ? -1 : 0;
        break;
      }
      case 3: reinterpret_cast<int64_t*>(out)[i] = lo + i; break;  // arange
      default: break;
    }
  }
}

extern "C" int bg_fill_rand(void* d_out, int64_t n, uint64_t seed,
                            int64_t lo, int64_t hi, int32_t mode) {
  REQUIRE_INIT();
  if (n <= 0) return BG_OK;
  if (hi <= lo) return set_err(BG_ERR_INVALID, "bg_fill_rand: hi <= lo");
  int blocks = (int)bg_imin64((n + BG_BLOCK - 1) / BG_BLOCK, BG_MAX_BLOCKS);
  hipLaunchKernelGGL(k_fill_rand, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (uint8_t*)d_out, n, seed, lo, (uint64_t)(hi - lo), mode);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Generalized HashJoinExec build/probe (round 2): multi-column keys over
// Int64/Int32/Date32/Decimal128/Utf8/dict8 and the non-inner join types
// DataFusion's HashJoinExec supports on the probe side (LeftSemi/LeftAnti/
// Left with the probe side as the preserved side — SURVEY.md §8a row 3;
// q2/q9-class shapes).  Nodes store {hash, next} (the general analogue of
// the Int64 path's {key, next}: full-hash reject before the cross-table
// key compare).  Join null semantics (null_equals_null=false): a row with
// ANY null key matches nothing — excluded from INNER/SEMI, EMITTED by
// ANTI and OUTER (with a BG_JOIN_NULL_IDX build id).
// ---------------------------------------------------------------------------

__device__ __forceinline__ bool row_has_null_key(const KeyArgs& keys,
                                                 int64_t i) {
  for (int c = 0; c < keys.nkeys; ++c)
    if (keys.k[c].valid && !bit_valid(keys.k[c].valid, i)) return true;
  return false;
}

// cross-table key equality (build row vs probe row); nulls already
// excluded by row_has_null_key
__device__ __forceinline__ bool keys_equal_cross(const KeyArgs& a, int64_t ra,
                                                 const KeyArgs& b,
                                                 int64_t rb) {
  for (int c = 0; c < a.nkeys; ++c) {
    switch (a.k[c].dtype) {
      case BG_DT_INT64:
        if (reinterpret_cast<const int64_t*>(a.k[c].data)[ra] !=
            reinterpret_cast<const int64_t*>(b.k[c].data)[rb])
          return false;
        break;
      case BG_DT_INT32:
      case BG_DT_DATE32:
        if (reinterpret_cast<const int32_t*>(a.k[c].data)[ra] !=
            reinterpret_cast<const int32_t*>(b.k[c].data)[rb])
          return false;
        break;
      case BG_DT_DECIMAL128: {
        const ulong2 x = reinterpret_cast<const ulong2*>(a.k[c].data)[ra];
        const ulong2 y = reinterpret_cast<const ulong2*>(b.k[c].data)[rb];
        if (x.x != y.x || x.y != y.y) return false;
        break;
      }
      case BG_DT_DICT8:
        if (reinterpret_cast<const uint8_t*>(a.k[c].data)[ra] !=
            reinterpret_cast<const uint8_t*>(b.k[c].data)[rb])
          return false;
        break;
      case BG_DT_UTF8: {
        const int32_t la = a.k[c].offsets[ra], ha = a.k[c].offsets[ra + 1];
        const int32_t lb = b.k[c].offsets[rb], hb = b.k[c].offsets[rb + 1];
        if (ha - la != hb - lb) return false;
        const uint8_t* da = reinterpret_cast<const uint8_t*>(a.k[c].data);
        const uint8_t* db = reinterpret_cast<const uint8_t*>(b.k[c].data);
        for (int32_t j = 0; j < ha - la; ++j)
          if (da[la + j] != db[lb + j]) return false;
        break;
      }
      default:
        return false;
    }
  }
  return true;
}

__global__ void k_join_build2(KeyArgs keys, int64_t n, int* head,
                              ulong2* nodes, u64 mask) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (row_has_null_key(keys, i)) continue;
    const u64 h = hash_keys_row(keys, i);
    const int prev = atomicExch(&head[h & mask], (int)i);
    ulong2 node;
    node.x = h;
    node.y = (u64)(int64_t)prev;
    nodes[i] = node;
  }
}

// Build-side-preserving types (DataFusion's LeftSemi/LeftAnti/Left/Full,
// build = its left input): one visited bit per build row, Arrow LSB order,
// set by every probe row that matches it.  The plain load in front of the
// atomic is only a hint (most marks are repeats: ~4 lineitems per order);
// bits are set-only after a zeroing memset, so a stale 0 costs one
// redundant atomicOr and a stale 1 cannot occur.  Readers are later
// kernels on the same stream; nothing reads the bitmap inside a launch.
__device__ __forceinline__ void mark_visited(uint32_t* words, int64_t row) {
  uint32_t* w = &words[row >> 5];
  const uint32_t bit = 1u << (row & 31);
  if (!(*w & bit)) atomicOr(w, bit);  // result unused: no-return form
}

// ---------------------------------------------------------------------------
// Join residual filters (HashJoinExec with filter: Some(JoinFilter);
// approved/q21.txt:60-61, q7.txt, q19.txt).  The filter decides which
// key-equal candidates count as matches, so it runs inside the chain walk,
// in front of the join type's bookkeeping.  It is an OR of groups, each an
// AND of: one bit of a build-side mask, one bit of a probe-side mask (the
// caller evaluated the single-side predicates into them) and up to four
// build-column <cmp> probe-column compares.  The program travels as a
// kernel argument like KeyArgs; every loop bound over it is wave-uniform.
// The probe kernels below take it through a filter policy, so the filtered
// and the unfiltered probe are two instantiations of one chain walk.
// ---------------------------------------------------------------------------
struct JoinFilterArgs {
  int ngroups;
  struct Group {
    const uint8_t* build_mask;  // Arrow LSB bits over build rows, or null
    const uint8_t* probe_mask;  // over this launch's probe rows, or null
    int ncross;
    struct Cross {
      const void* b;
      const uint8_t* bvalid;
      const void* p;
      const uint8_t* pvalid;
      int dtype;
      int cmp;
    } x[BG_JOIN_FILTER_MAX_CROSS];
  } g[BG_JOIN_FILTER_MAX_GROUPS];
};

template <typename T>
__device__ __forceinline__ bool jf_compare(T x, T y, int cmp) {
  switch (cmp) {
    case BG_CMP_LT: return x < y;
    case BG_CMP_LE: return x <= y;
    case BG_CMP_GT: return x > y;
    case BG_CMP_GE: return x >= y;
    case BG_CMP_EQ: return x == y;
    default: return x != y;  // BG_CMP_NE (host checked the range)
  }
}

// one cross term: validity first (NULL on either side fails the term),
// Decimal128 as signed i128 like cmp_load<i128>
__device__ __forceinline__ bool jf_cross_passes(
    const JoinFilterArgs::Group::Cross& x, int64_t b, int64_t p) {
  if (!bit_valid(x.bvalid, b) || !bit_valid(x.pvalid, p)) return false;
  switch (x.dtype) {
    case BG_DT_INT64:
      return jf_compare(reinterpret_cast<const int64_t*>(x.b)[b],
                        reinterpret_cast<const int64_t*>(x.p)[p], x.cmp);
    case BG_DT_INT32:
    case BG_DT_DATE32:
      return jf_compare(reinterpret_cast<const int32_t*>(x.b)[b],
                        reinterpret_cast<const int32_t*>(x.p)[p], x.cmp);
    case BG_DT_DICT8:
      return jf_compare(reinterpret_cast<const uint8_t*>(x.b)[b],
                        reinterpret_cast<const uint8_t*>(x.p)[p], x.cmp);
    case BG_DT_DECIMAL128:
      return jf_compare(load_dec128(x.b, b), load_dec128(x.p, p), x.cmp);
    default:
      return false;  // the host refuses every other dtype
  }
}

// the groups whose probe-side mask keeps probe row p; 0 = no candidate of
// this row can pass, whatever its key
__device__ __forceinline__ uint32_t jf_live_groups(const JoinFilterArgs& f,
                                                   int64_t p) {
  uint32_t live = 0;
  for (int g = 0; g < f.ngroups; ++g)
    if (bit_valid(f.g[g].probe_mask, p)) live |= 1u << g;
  return live;
}

// THE decision "candidate (build row b, probe row p) passes", called from
// the one chain walk (join_walk) that count, fill and mark share, so they
// cannot disagree (count sizes the slots fill writes into).  First failing
// term ends a group, first passing group ends the test.
__device__ __forceinline__ bool jf_candidate_passes(const JoinFilterArgs& f,
                                                    uint32_t live, int64_t b,
                                                    int64_t p) {
  for (int g = 0; g < f.ngroups; ++g) {
    if (!((live >> g) & 1)) continue;
    if (!bit_valid(f.g[g].build_mask, b)) continue;
    int c = 0;
    while (c < f.g[g].ncross && jf_cross_passes(f.g[g].x[c], b, p)) ++c;
    if (c == f.g[g].ncross) return true;
  }
  return false;
}

// Filter policies of the chain walk.  live(p): the groups probe row p can
// still pass in, 0 = skip the row; passes(live, b, p): candidate (b, p)
// counts as a match.  JoinNoFilter is empty, so the unfiltered kernels carry
// no JoinFilterArgs in their argument block.
struct JoinNoFilter {
  __device__ __forceinline__ uint32_t live(int64_t) const { return 1; }
  __device__ __forceinline__ bool passes(uint32_t, int64_t, int64_t) const {
    return true;
  }
};
struct JoinFiltered {
  JoinFilterArgs f;
  __device__ __forceinline__ uint32_t live(int64_t p) const {
    return jf_live_groups(f, p);
  }
  __device__ __forceinline__ bool passes(uint32_t live, int64_t b,
                                         int64_t p) const {
    return jf_candidate_passes(f, live, b, p);
  }
};

// The table a probe kernel walks and the probe rows it walks it for.
struct JoinProbeArgs {
  KeyArgs bkeys, pkeys;
  int64_t n_probe;
  const int* head;
  const ulong2* nodes;
  u64 mask;
};

// THE chain walk of probe row i: calls match(build row) for every build row
// with an equal key that the filter passes, in chain order, until match
// returns true ("stop").  A probe row with no live group or with a NULL key
// matches nothing and is neither hashed nor walked.  Count, fill and mark
// all go through here, so they see the same matches in the same order.
// The stop flag in the loop condition, not an early return, is deliberate:
// with a return the unfiltered fill compiles to 106 SGPRs and 7 waves, with
// the flag to 100 and 8 (profiles/kernel_resource_usage_join_probe.txt).
template <typename Filter, typename Match>
__device__ __forceinline__ void join_walk(const JoinProbeArgs& t,
                                          const Filter& f, int64_t i,
                                          Match&& match) {
  const uint32_t live = f.live(i);
  if (!live || row_has_null_key(t.pkeys, i)) return;
  const u64 h = hash_keys_row(t.pkeys, i);
  int64_t cur = t.head[h & t.mask];
  bool stop = false;
  while (cur >= 0 && !stop) {
    const ulong2 node = t.nodes[cur];
    if (node.x == h && keys_equal_cross(t.bkeys, cur, t.pkeys, i) &&
        f.passes(live, cur, i))
      stop = match(cur);
    cur = (int64_t)node.y;
  }
}

// What the four pair-emitting types do with a probe row (join_pair_type
// maps the marking types onto them before a launch).  The count and the fill
// both read these, so the fill writes exactly the slots the count sized.
__device__ __forceinline__ bool join_first_match_decides(int32_t jt) {
  return jt == BG_JOIN_SEMI || jt == BG_JOIN_ANTI;
}
__device__ __forceinline__ bool join_emits_matches(int32_t jt) {
  return jt != BG_JOIN_ANTI;
}
__device__ __forceinline__ bool join_emits_unmatched_probe(int32_t jt) {
  return jt == BG_JOIN_ANTI || jt == BG_JOIN_OUTER_PROBE;
}

// ---------------------------------------------------------------------------
// Nested-loop join (NestedLoopJoinExec, datafusion.proto:1359-1365;
// approved/q11.txt:69, q22.txt:14): a join without keys, so EVERY build row
// is a candidate of every probe row and the residual filter alone decides.
// It is the general probe with a plain loop over the build rows in place of
// the chain walk: the same probe kernels (below, over a walk policy), the
// same filter policies, the same count -> exclusive scan -> fill scheme and
// the same visited bitmap.
//
// Lanes own probe rows; the build index b runs 0 .. n_build-1 in a loop
// whose control is wave-uniform, so a build row's mask bit, value and
// validity sit at one address per wave, and the probe row's operands do not
// change across the loop.  Whole waves iterate: a lane past n_probe stays
// in with active = false, which makes marking build row b one ballot and one
// mark_visited by lane 0 instead of up to 64 lanes contending on one word.
// Parallelism is over probe rows only: a one-row probe side against a large
// build side runs serially in one lane (DataFusion puts the smaller input
// on the build side, so the approved plans never have that shape).
// ---------------------------------------------------------------------------

// the groups some lane of this wave is still live in
__device__ __forceinline__ uint32_t jf_wave_groups(int ngroups, uint32_t live) {
  uint32_t any = 0;
  for (int g = 0; g < ngroups; ++g)
    if (__ballot((live >> g) & 1) != 0) any |= 1u << g;
  return any;
}

// What the nested-loop walk asks of a filter policy beyond live() and
// passes(): the groups live anywhere in the wave (0 = the wave walks
// nothing), and whether build row b can pass in one of them, which is one
// wave-uniform test because b is.
__device__ __forceinline__ uint32_t nl_wave_groups(const JoinNoFilter&,
                                                   uint32_t live) {
  return __ballot(live != 0) != 0;
}
__device__ __forceinline__ uint32_t nl_wave_groups(const JoinFiltered& f,
                                                   uint32_t live) {
  return jf_wave_groups(f.f.ngroups, live);
}
__device__ __forceinline__ bool nl_build_live(const JoinNoFilter&, uint32_t,
                                              int64_t) {
  return true;
}
__device__ __forceinline__ bool nl_build_live(const JoinFiltered& f,
                                              uint32_t groups, int64_t b) {
  for (int g = 0; g < f.f.ngroups; ++g)
    if (((groups >> g) & 1) && bit_valid(f.f.g[g].build_mask, b)) return true;
  return false;
}

// THE nested-loop walk of probe row i (active: i is a row of this launch):
// calls match(build row) for every build row the filter passes, in ascending
// build order, until match returns true ("stop"), the contract of join_walk.
// Every lane of the wave must call it; the wave leaves the loop when no lane
// still wants candidates.  A probe row with no live group walks nothing, a
// build row whose masks clear every group live in the wave is skipped by
// all of it.  There are no keys, so the only NULL rule is the filter's.
// MARK sets the visited bit of every build row some lane matched.  Count,
// fill and mark all go through here, so they see the same matches in the
// same order.
template <bool MARK, typename Filter, typename Match>
__device__ __forceinline__ void nl_join_walk(int64_t n_build, const Filter& f,
                                             int64_t i, bool active,
                                             uint32_t* visited,
                                             Match&& match) {
  const uint32_t live = active ? f.live(i) : 0;
  bool want = live != 0;
  const uint32_t groups = nl_wave_groups(f, live);
  if (!groups) return;
  for (int64_t b = 0; b < n_build && __ballot(want) != 0; ++b) {
    if (!nl_build_live(f, groups, b)) continue;
    const bool hit = want && f.passes(live, b, i);
    if (MARK && __ballot(hit) != 0 && lane_id() == 0)
      mark_visited(visited, b);
    if (hit) want = !match(b);
  }
}

struct NlJoinArgs {
  int64_t n_build, n_probe;
};

// Walk policies of the probe kernels: where the candidates of a probe row
// come from, and with them how a kernel's lanes step through the probe rows,
// because the two walks ask different things of that loop.
//   rows(first, stride, fn)
//              calls fn(i, active) for the probe rows of this lane; active
//              is false where the lane is only kept in for its wave.  first
//              is the block's first row and stride the grid's rows per step:
//              the kernel reads them, because blockDim read in a member
//              function is loaded per lane (+2 VGPRs in every instantiation,
//              profiles/kernel_resource_usage_join_walk.txt).
//   walk<MARK> calls match(build row) for every match of probe row i, in the
//              walk's order, until match returns true ("stop"); MARK also
//              sets the visited bit of every build row it reports.
// The hash walk steps per lane: a lane past n_probe simply leaves, and
// nothing a lane of JoinHashWalk reaches may hold a ballot.
struct JoinHashWalk {
  JoinProbeArgs t;
  template <typename Fn>
  __device__ __forceinline__ void rows(int64_t first, int64_t stride,
                                       Fn&& fn) const {
    for (int64_t i = first + threadIdx.x; i < t.n_probe; i += stride)
      fn(i, true);
  }
  template <bool MARK, typename Filter, typename Match>
  __device__ __forceinline__ void walk(const Filter& f, int64_t i, bool,
                                       uint32_t* visited, Match&& match) const {
    join_walk(t, f, i, [&](int64_t b) {
      if (MARK) mark_visited(visited, b);
      return match(b);
    });
  }
};
// The nested-loop walk steps by whole blocks, so every wave enters
// nl_join_walk complete: a lane past n_probe stays in with active = false.
// Marking is nl_join_walk<MARK>'s own (one ballot per build row).
struct JoinNlWalk {
  NlJoinArgs t;
  template <typename Fn>
  __device__ __forceinline__ void rows(int64_t first, int64_t stride,
                                       Fn&& fn) const {
    for (int64_t base = first; base < t.n_probe; base += stride) {
      const int64_t i = base + threadIdx.x;
      fn(i, i < t.n_probe);
    }
  }
  template <bool MARK, typename Filter, typename Match>
  __device__ __forceinline__ void walk(const Filter& f, int64_t i, bool active,
                                       uint32_t* visited, Match&& match) const {
    nl_join_walk<MARK>(t.n_build, f, i, active, visited, match);
  }
};

// THE probe kernels of the general hash join and of the nested-loop join.
// What a join type does with a match, with an unmatched probe row and when
// its walk may stop is written here once per phase, for both walks and both
// filter policies.  Pair order: ascending probe row; within a probe row the
// walk's order (chain order, or ascending build row for the nested loop); an
// unmatched probe row (ANTI / OUTER_PROBE) carries BG_JOIN_NULL_IDX.
template <typename Walk, typename Filter>
__global__ void k_join_count2(Walk w, int32_t join_type, Filter f,
                              uint32_t* counts) {
  const int64_t first = (int64_t)blockIdx.x * blockDim.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  w.rows(first, stride, [&](int64_t i, bool active) {
    u64 cnt = 0;
    w.template walk<false>(f, i, active, nullptr, [&](int64_t) {
      ++cnt;
      return join_first_match_decides(join_type);
    });
    if (!join_emits_matches(join_type)) cnt = cnt ? 0 : 1;
    else if (join_emits_unmatched_probe(join_type)) cnt = cnt ? cnt : 1;
    if (active) counts[i] = (uint32_t)cnt;
  });
}

// Writes the pairs k_join_count2 counted for the same join_type and filter.
// MARK also marks every matched build row; it is launched for INNER and
// OUTER_PROBE pairs only, so the first-match types compile out of it.
template <typename Walk, typename Filter, bool MARK>
__global__ void k_join_fill2(Walk w, int32_t join_type, Filter f,
                             const i64* offsets, uint32_t* out_probe,
                             uint32_t* out_build, uint32_t* visited) {
  const int64_t first = (int64_t)blockIdx.x * blockDim.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  w.rows(first, stride, [&](int64_t i, bool active) {
    i64 slot = active ? offsets[i] : 0;
    bool matched = false;
    w.template walk<MARK>(f, i, active, visited, [&](int64_t b) {
      matched = true;
      if (!MARK && !join_emits_matches(join_type)) return true;
      out_probe[slot] = (uint32_t)i;
      out_build[slot] = (uint32_t)b;
      ++slot;
      return !MARK && join_first_match_decides(join_type);
    });
    if (active && !matched && join_emits_unmatched_probe(join_type)) {
      out_probe[slot] = (uint32_t)i;
      out_build[slot] = BG_JOIN_NULL_IDX;
    }
  });
}

// Marks every matched build row and emits nothing: walks every candidate.
template <typename Walk, typename Filter>
__global__ void k_join_mark2(Walk w, Filter f, uint32_t* visited) {
  const int64_t first = (int64_t)blockIdx.x * blockDim.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  w.rows(first, stride, [&](int64_t i, bool active) {
    w.template walk<true>(f, i, active, visited,
                          [](int64_t) { return false; });
  });
}

// ~visited (or all ones where nothing was ever marked) as a mask for the
// stable compaction, which trims the bits at or beyond n itself
__global__ void k_bitmap_not_u64(const u64* in, int64_t nwords, u64* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = in ? ~in[i] : ~0ull;
}

static int keyargs_from_cols(const bg_column* cols, int32_t nkeys,
                             KeyArgs* out) {
  if (nkeys <= 0 || nkeys > BG_MAX_KEYS) return BG_ERR_INVALID;
  out->nkeys = nkeys;
  for (int c = 0; c < nkeys; ++c) {
    out->k[c].data = cols[c].d_data;
    out->k[c].valid = cols[c].d_validity;
    out->k[c].offsets = cols[c].d_offsets;
    out->k[c].dtype = cols[c].dtype;
    switch (cols[c].dtype) {
      case BG_DT_INT64:
      case BG_DT_INT32:
      case BG_DT_DATE32:
      case BG_DT_DECIMAL128:
      case BG_DT_DICT8:
      case BG_DT_UTF8:
        break;
      default:
        return BG_ERR_UNSUPPORTED;
    }
  }
  return BG_OK;
}

// What a handle keeps between its probe calls: the offsets between a count
// and its fill, and the visited bitmap.  The nested-loop handle is this and
// nothing more; the general hash handle adds its table and keys.
struct JoinProbeState {
  int64_t n_build = 0;
  i64* probe_offsets = nullptr;
  int64_t probe_n = 0;
  int32_t probe_jt = -1;
  // one visited bit per build row, ((n_build+63)/64)*8 + 8 bytes; allocated
  // and zeroed by the first marking call, accumulated until the handle's free
  uint32_t* visited = nullptr;
  // the filter of the last filtered count, which stores probe_jt with
  // JOIN_JT_FILTERED set: a fill must repeat both
  JoinFilterArgs probe_filter = {};
};
#define JOIN_JT_FILTERED 0x100
struct BgJoinTable2 : JoinProbeState {
  ulong2* nodes;
  int* head;
  u64 mask;
  KeyArgs bkeys;  // caller's device buffers must outlive the handle
  int32_t nkeys;
};
using BgNlJoin = JoinProbeState;

// The wording of the shared checks, which names each handle's own entries.
struct JoinHandleText {
  const char* count_first;           // a fill no unfiltered count sized
  const char* count_first_filtered;  // a fill no filtered count sized
  const char* no_pairs;              // SEMI_BUILD / ANTI_BUILD to count or fill
};
static const JoinHandleText kHashJoinText = {
    "call bg_hashjoin_probe_count2 first (same join_type)",
    "call bg_hashjoin_probe_count2_filtered first (same join_type, same "
    "terms)",
    "SEMI_BUILD/ANTI_BUILD emit no pairs: call bg_hashjoin_probe_mark2, then "
    "bg_hashjoin_build_rows2"};
static const JoinHandleText kNlJoinText = {
    "call bg_nljoin_count first (same n_probe, same join_type, same terms)",
    "call bg_nljoin_count first (same n_probe, same join_type, same terms)",
    "SEMI_BUILD/ANTI_BUILD emit no pairs: call bg_nljoin_mark, then "
    "bg_nljoin_build_rows"};

static inline uint64_t join_visited_bytes(int64_t n_build) {
  return (uint64_t)((n_build + 63) / 64) * 8 + 8;
}

// lazily allocate + zero the visited bitmap (stream-ordered memset: every
// marking kernel is launched on the same null stream after it)
static int join_ensure_visited(JoinProbeState* t) {
  if (t->visited) return BG_OK;
  DevBuf<uint8_t> v;
  HIP_TRY(v.alloc((int64_t)join_visited_bytes(t->n_build)));
  HIP_TRY(hipMemsetAsync(v, 0, join_visited_bytes(t->n_build), 0));
  t->visited = reinterpret_cast<uint32_t*>(v.detach());
  return BG_OK;
}

// what either handle's free gives back to the pool for the probe state
static void join_release_probe_state(JoinProbeState* t) {
  if (t->probe_offsets) (void)pool_release(t->probe_offsets);
  if (t->visited) (void)pool_release(t->visited);
}

// probe keys checked against the handle's build keys
static int join_probe_keys(const BgJoinTable2* t, const bg_column* keys,
                           int32_t nkeys, KeyArgs* pk) {
  if (nkeys != t->nkeys)
    return set_err(BG_ERR_INVALID, "probe/build key counts differ");
  // a dtype keyargs_from_cols refuses is none of the build's either
  bool same = keyargs_from_cols(keys, nkeys, pk) == BG_OK;
  for (int c = 0; same && c < nkeys; ++c)
    same = pk->k[c].dtype == t->bkeys.k[c].dtype;
  if (!same) return set_err(BG_ERR_INVALID, "probe/build key dtypes differ");
  return BG_OK;
}

// The count and fill entries take the pair-emitting types only: SEMI_BUILD /
// ANTI_BUILD emit build rows, never pairs.
static int join_check_pair_type(int32_t jt, const JoinHandleText& text) {
  if (jt == BG_JOIN_SEMI_BUILD || jt == BG_JOIN_ANTI_BUILD)
    return set_err(BG_ERR_INVALID, text.no_pairs);
  if (jt < BG_JOIN_INNER || jt > BG_JOIN_OUTER_FULL)
    return set_err(BG_ERR_INVALID, "unknown join_type");
  return BG_OK;
}

// The marking types emit the pairs of the type they extend: OUTER_BUILD
// pairs as INNER, OUTER_FULL pairs as OUTER_PROBE.
static int32_t join_pair_type(int32_t jt) {
  return jt == BG_JOIN_OUTER_BUILD  ? BG_JOIN_INNER
         : jt == BG_JOIN_OUTER_FULL ? BG_JOIN_OUTER_PROBE
                                    : jt;
}
static bool join_type_marks(int32_t jt) {
  return jt == BG_JOIN_OUTER_BUILD || jt == BG_JOIN_OUTER_FULL;
}

extern "C" int bg_hashjoin_build2(const bg_column* keys, int32_t nkeys,
                                  int64_t n, void** out_handle) {
  REQUIRE_INIT();
  if (n > 0x7fffffffLL)
    return set_err(BG_ERR_INVALID, "build side > 2^31 rows");
  BgJoinTable2 t{};
  if (keyargs_from_cols(keys, nkeys, &t.bkeys) != BG_OK)
    return set_err(BG_ERR_UNSUPPORTED, "join key dtype/count unsupported");
  t.nkeys = nkeys;
  t.n_build = n;
  DevBuf<ulong2> nodes;
  DevBuf<int> head;
  int rc = join_alloc_table(n, &t.mask, &head, &nodes);
  if (rc != BG_OK) return rc;
  int blocks = grid_for(n);
  hipLaunchKernelGGL(k_join_build2, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     t.bkeys, n, head.get(), nodes.get(), t.mask);
  HIP_TRY(hipGetLastError());
  // the handle owns the table from here; bg_hashjoin_free2 releases it
  t.nodes = nodes.detach();
  t.head = head.detach();
  *out_handle = new BgJoinTable2(t);
  return BG_OK;
}

extern "C" int bg_hashjoin_free2(void* handle) {
  REQUIRE_INIT();
  BgJoinTable2* t = (BgJoinTable2*)handle;
  if (!t) return BG_OK;
  (void)pool_release(t->nodes);
  (void)pool_release(t->head);
  join_release_probe_state(t);
  delete t;
  return BG_OK;
}

// The build rows of either visited-bitmap handle whose bit == matched, in
// ascending build order; bits at or beyond n_build are never reported.
static int join_build_rows(JoinProbeState* t, int32_t matched,
                           int64_t* out_count, uint32_t* d_out_build) {
  if (!t || !out_count)
    return set_err(BG_ERR_INVALID, "null join handle / out_count");
  if (matched != 0 && matched != 1)
    return set_err(BG_ERR_INVALID, "matched must be 0 or 1");
  *out_count = 0;
  // nothing marked yet: no build row is matched
  if (t->n_build == 0 || (matched && !t->visited)) return BG_OK;
  if (matched)
    return mask_to_indices(reinterpret_cast<const uint8_t*>(t->visited),
                           t->n_build, d_out_build, out_count);
  const int64_t nwords = (t->n_build + 63) / 64;
  DevBuf<u64> inv;
  HIP_TRY(inv.alloc(nwords));
  hipLaunchKernelGGL(k_bitmap_not_u64, dim3(grid_for(nwords)),
                     dim3(BG_BLOCK), 0, 0,
                     reinterpret_cast<const u64*>(t->visited), nwords,
                     inv.get());
  HIP_TRY(hipGetLastError());
  return mask_to_indices(reinterpret_cast<const uint8_t*>(inv.get()),
                         t->n_build, d_out_build, out_count);
}

extern "C" int bg_hashjoin_build_rows2(void* handle, int32_t matched,
                                       int64_t* out_count,
                                       uint32_t* d_out_build) {
  REQUIRE_INIT();
  return join_build_rows((BgJoinTable2*)handle, matched, out_count,
                         d_out_build);
}

// flat ABI terms -> the kernels' grouped program, every limit checked
static int join_filter_args(const bg_join_filter_term* terms, int32_t nterms,
                            int64_t n_build, int64_t n_probe,
                            JoinFilterArgs* f) {
  if (nterms <= 0 || !terms)
    return set_err(BG_ERR_INVALID,
                   "join filter: no terms (a join without a filter goes "
                   "through the unfiltered entries)");
  memset(f, 0, sizeof(*f));
  bool seen[BG_JOIN_FILTER_MAX_GROUPS] = {};
  for (int32_t i = 0; i < nterms; ++i) {
    const bg_join_filter_term& t = terms[i];
    if (t.group < 0 || t.group >= BG_JOIN_FILTER_MAX_GROUPS)
      return set_err(BG_ERR_INVALID, "join filter: group id outside [0,4)");
    JoinFilterArgs::Group& g = f->g[t.group];
    seen[t.group] = true;
    if (t.group + 1 > f->ngroups) f->ngroups = t.group + 1;
    switch (t.kind) {
      case BG_JF_BUILD_MASK:
        if (!t.d_build || g.build_mask)
          return set_err(BG_ERR_INVALID,
                         "join filter: null or second build mask in a group");
        g.build_mask = reinterpret_cast<const uint8_t*>(t.d_build);
        break;
      case BG_JF_PROBE_MASK:
        if (!t.d_probe || g.probe_mask)
          return set_err(BG_ERR_INVALID,
                         "join filter: null or second probe mask in a group");
        g.probe_mask = reinterpret_cast<const uint8_t*>(t.d_probe);
        break;
      case BG_JF_CROSS: {
        if (t.cmp < BG_CMP_LT || t.cmp > BG_CMP_NE)
          return set_err(BG_ERR_INVALID, "join filter: unknown cmp");
        if (t.dtype == BG_DT_FLOAT64 || t.dtype == BG_DT_UTF8)
          return set_err(BG_ERR_UNSUPPORTED,
                         "join filter: cross compare of Float64/Utf8 columns");
        if (t.dtype != BG_DT_INT32 && t.dtype != BG_DT_INT64 &&
            t.dtype != BG_DT_DATE32 && t.dtype != BG_DT_DECIMAL128 &&
            t.dtype != BG_DT_DICT8)
          return set_err(BG_ERR_INVALID, "join filter: unknown dtype");
        // an empty side may come without buffers; nothing indexes it
        if ((!t.d_build && n_build > 0) || (!t.d_probe && n_probe > 0))
          return set_err(BG_ERR_INVALID, "join filter: null cross column");
        if (g.ncross == BG_JOIN_FILTER_MAX_CROSS)
          return set_err(BG_ERR_INVALID,
                         "join filter: more than 4 cross terms in a group");
        JoinFilterArgs::Group::Cross& x = g.x[g.ncross++];
        x.b = t.d_build;
        x.bvalid = t.d_build_validity;
        x.p = t.d_probe;
        x.pvalid = t.d_probe_validity;
        x.dtype = t.dtype;
        x.cmp = t.cmp;
        break;
      }
      default:
        return set_err(BG_ERR_INVALID, "join filter: unknown term kind");
    }
  }
  for (int g = 0; g < f->ngroups; ++g)
    if (!seen[g])
      return set_err(BG_ERR_INVALID,
                     "join filter: group ids must be dense from 0 (an empty "
                     "group would pass everything)");
  return BG_OK;
}

// run(policy) with the walk's filter policy for an optional filter
template <typename Run>
static void join_with_filter(const JoinFilterArgs* f, Run&& run) {
  if (f) run(JoinFiltered{*f});
  else run(JoinNoFilter{});
}

// Count, fill and mark of a checked call on either handle: w is the handle's
// walk over this call's probe rows, f is null without a filter.
template <typename Walk>
static int join_count(JoinProbeState* t, const Walk& w, int32_t join_type,
                      const JoinFilterArgs* f, int64_t* out_matches) {
  if (!out_matches) return set_err(BG_ERR_INVALID, "null out_matches");
  const int64_t n = w.t.n_probe;
  int rc = join_count_phase(t, n, out_matches, [&](uint32_t* counts) {
    join_with_filter(f, [&](auto filter) {
      hipLaunchKernelGGL((k_join_count2<Walk, decltype(filter)>),
                         dim3(grid_for(n)), dim3(BG_BLOCK), 0, 0, w,
                         join_pair_type(join_type), filter, counts);
    });
  });
  if (rc != BG_OK) return rc;
  // a fill must repeat the type and, with JOIN_JT_FILTERED, the filter
  t->probe_jt = f ? join_type | JOIN_JT_FILTERED : join_type;
  if (f) t->probe_filter = *f;
  return BG_OK;
}

template <typename Walk>
static int join_fill(JoinProbeState* t, const Walk& w, int32_t join_type,
                     const JoinFilterArgs* f, const JoinHandleText& text,
                     uint32_t* d_out_probe, uint32_t* d_out_build) {
  const int64_t n = w.t.n_probe;
  // the offsets are only good for the type and filter they were counted under
  if (!t->probe_offsets || t->probe_n != n ||
      t->probe_jt != (f ? join_type | JOIN_JT_FILTERED : join_type) ||
      (f && memcmp(f, &t->probe_filter, sizeof(*f)) != 0))
    return set_err(BG_ERR_INVALID,
                   f ? text.count_first_filtered : text.count_first);
  const bool mark = join_type_marks(join_type);
  if (mark) {
    int rc = join_ensure_visited(t);
    if (rc != BG_OK) return rc;
  }
  join_with_filter(f, [&](auto filter) {
    using F = decltype(filter);
    hipLaunchKernelGGL(
        (mark ? k_join_fill2<Walk, F, true> : k_join_fill2<Walk, F, false>),
        dim3(grid_for(n)), dim3(BG_BLOCK), 0, 0, w, join_pair_type(join_type),
        filter, t->probe_offsets, d_out_probe, d_out_build, t->visited);
  });
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

template <typename Walk>
static int join_mark(JoinProbeState* t, const Walk& w,
                     const JoinFilterArgs* f) {
  int rc = join_ensure_visited(t);
  if (rc != BG_OK) return rc;
  const int64_t n = w.t.n_probe;
  if (n <= 0) return BG_OK;
  join_with_filter(f, [&](auto filter) {
    hipLaunchKernelGGL((k_join_mark2<Walk, decltype(filter)>),
                       dim3(grid_for(n)), dim3(BG_BLOCK), 0, 0, w, filter,
                       t->visited);
  });
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// What every general hash probe entry checks first, before anything is
// allocated or launched: the handle, the probe keys against the build's,
// the pair type of a count or fill (pair_type null: a mark entry, which has
// none) and, for a _filtered entry (f not null), its terms.  -> the walk over
// this call's probe rows and, filtered, the filter.
static int hashjoin_check(void* handle, const bg_column* keys, int32_t nkeys,
                          int64_t n, const int32_t* pair_type,
                          const bg_join_filter_term* terms, int32_t nterms,
                          JoinHashWalk* w, JoinFilterArgs* f) {
  const BgJoinTable2* t = (const BgJoinTable2*)handle;
  if (!t) return set_err(BG_ERR_INVALID, "null join handle");
  w->t.bkeys = t->bkeys;
  w->t.n_probe = n;
  w->t.head = t->head;
  w->t.nodes = t->nodes;
  w->t.mask = t->mask;
  int rc = join_probe_keys(t, keys, nkeys, &w->t.pkeys);
  if (rc == BG_OK && pair_type)
    rc = join_check_pair_type(*pair_type, kHashJoinText);
  if (rc == BG_OK && f)
    rc = join_filter_args(terms, nterms, t->n_build, n, f);
  return rc;
}

extern "C" int bg_hashjoin_probe_count2(void* handle, const bg_column* keys,
                                        int32_t nkeys, int64_t n,
                                        int32_t join_type,
                                        int64_t* out_matches) {
  REQUIRE_INIT();
  JoinHashWalk w;
  int rc = hashjoin_check(handle, keys, nkeys, n, &join_type, nullptr, 0, &w,
                          nullptr);
  if (rc != BG_OK) return rc;
  return join_count((BgJoinTable2*)handle, w, join_type, nullptr, out_matches);
}

extern "C" int bg_hashjoin_probe_fill2(void* handle, const bg_column* keys,
                                       int32_t nkeys, int64_t n,
                                       int32_t join_type,
                                       uint32_t* d_out_probe,
                                       uint32_t* d_out_build) {
  REQUIRE_INIT();
  JoinHashWalk w;
  int rc = hashjoin_check(handle, keys, nkeys, n, &join_type, nullptr, 0, &w,
                          nullptr);
  if (rc != BG_OK) return rc;
  return join_fill((BgJoinTable2*)handle, w, join_type, nullptr,
                   kHashJoinText, d_out_probe, d_out_build);
}

extern "C" int bg_hashjoin_probe_mark2(void* handle, const bg_column* keys,
                                       int32_t nkeys, int64_t n) {
  REQUIRE_INIT();
  JoinHashWalk w;
  int rc = hashjoin_check(handle, keys, nkeys, n, nullptr, nullptr, 0, &w,
                          nullptr);
  if (rc != BG_OK) return rc;
  return join_mark((BgJoinTable2*)handle, w, nullptr);
}

extern "C" int bg_hashjoin_probe_count2_filtered(
    void* handle, const bg_column* keys, int32_t nkeys, int64_t n,
    int32_t join_type, const bg_join_filter_term* terms, int32_t nterms,
    int64_t* out_matches) {
  REQUIRE_INIT();
  JoinHashWalk w;
  JoinFilterArgs f;
  int rc = hashjoin_check(handle, keys, nkeys, n, &join_type, terms, nterms,
                          &w, &f);
  if (rc != BG_OK) return rc;
  return join_count((BgJoinTable2*)handle, w, join_type, &f, out_matches);
}

extern "C" int bg_hashjoin_probe_fill2_filtered(
    void* handle, const bg_column* keys, int32_t nkeys, int64_t n,
    int32_t join_type, const bg_join_filter_term* terms, int32_t nterms,
    uint32_t* d_out_probe, uint32_t* d_out_build) {
  REQUIRE_INIT();
  JoinHashWalk w;
  JoinFilterArgs f;
  int rc = hashjoin_check(handle, keys, nkeys, n, &join_type, terms, nterms,
                          &w, &f);
  if (rc != BG_OK) return rc;
  return join_fill((BgJoinTable2*)handle, w, join_type, &f, kHashJoinText,
                   d_out_probe, d_out_build);
}

extern "C" int bg_hashjoin_probe_mark2_filtered(
    void* handle, const bg_column* keys, int32_t nkeys, int64_t n,
    const bg_join_filter_term* terms, int32_t nterms) {
  REQUIRE_INIT();
  JoinHashWalk w;
  JoinFilterArgs f;
  int rc = hashjoin_check(handle, keys, nkeys, n, nullptr, terms, nterms, &w,
                          &f);
  if (rc != BG_OK) return rc;
  return join_mark((BgJoinTable2*)handle, w, &f);
}

// ---- nested-loop join: host side ----

// What every bg_nljoin_* probe entry checks first, before anything is
// allocated or launched; terms == none (nterms 0) is a cross join.  pair_type
// as in hashjoin_check.  -> the walk over this call's probe rows and the
// filter, null for a cross join (*f is its storage).
static int nljoin_check(void* handle, int64_t n_probe,
                        const bg_join_filter_term* terms, int32_t nterms,
                        const int32_t* pair_type, JoinNlWalk* w,
                        JoinFilterArgs* f, const JoinFilterArgs** filter) {
  const BgNlJoin* t = (const BgNlJoin*)handle;
  if (!t) return set_err(BG_ERR_INVALID, "null nested-loop join handle");
  if (n_probe < 0)
    return set_err(BG_ERR_INVALID, "nested-loop join: negative n_probe");
  if (nterms < 0)
    return set_err(BG_ERR_INVALID, "nested-loop join: negative nterms");
  w->t = NlJoinArgs{t->n_build, n_probe};
  *filter = nterms > 0 ? f : nullptr;
  int rc = BG_OK;
  if (nterms > 0) rc = join_filter_args(terms, nterms, t->n_build, n_probe, f);
  if (rc == BG_OK && pair_type)
    rc = join_check_pair_type(*pair_type, kNlJoinText);
  return rc;
}

extern "C" int bg_nljoin_open(int64_t n_build, void** out_handle) {
  REQUIRE_INIT();
  if (!out_handle) return set_err(BG_ERR_INVALID, "null out_handle");
  if (n_build < 0)
    return set_err(BG_ERR_INVALID, "nested-loop join: negative n_build");
  // build rows travel as u32 indices and BG_JOIN_NULL_IDX is taken
  if (n_build >= 0xFFFFFFFFLL)
    return set_err(BG_ERR_INVALID,
                   "nested-loop join: build side >= 2^32 - 1 rows");
  BgNlJoin* t = new BgNlJoin();
  t->n_build = n_build;
  *out_handle = t;
  return BG_OK;
}

extern "C" int bg_nljoin_free(void* handle) {
  REQUIRE_INIT();
  BgNlJoin* t = (BgNlJoin*)handle;
  if (!t) return BG_OK;
  join_release_probe_state(t);
  delete t;
  return BG_OK;
}

extern "C" int bg_nljoin_count(void* handle, int64_t n_probe,
                               int32_t join_type,
                               const bg_join_filter_term* terms,
                               int32_t nterms, int64_t* out_matches) {
  REQUIRE_INIT();
  JoinNlWalk w;
  JoinFilterArgs f;
  const JoinFilterArgs* filter;
  int rc = nljoin_check(handle, n_probe, terms, nterms, &join_type, &w, &f,
                        &filter);
  if (rc != BG_OK) return rc;
  return join_count((BgNlJoin*)handle, w, join_type, filter, out_matches);
}

extern "C" int bg_nljoin_fill(void* handle, int64_t n_probe,
                              int32_t join_type,
                              const bg_join_filter_term* terms,
                              int32_t nterms, uint32_t* d_out_probe,
                              uint32_t* d_out_build) {
  REQUIRE_INIT();
  JoinNlWalk w;
  JoinFilterArgs f;
  const JoinFilterArgs* filter;
  int rc = nljoin_check(handle, n_probe, terms, nterms, &join_type, &w, &f,
                        &filter);
  if (rc != BG_OK) return rc;
  return join_fill((BgNlJoin*)handle, w, join_type, filter, kNlJoinText,
                   d_out_probe, d_out_build);
}

extern "C" int bg_nljoin_mark(void* handle, int64_t n_probe,
                              const bg_join_filter_term* terms,
                              int32_t nterms) {
  REQUIRE_INIT();
  JoinNlWalk w;
  JoinFilterArgs f;
  const JoinFilterArgs* filter;
  int rc = nljoin_check(handle, n_probe, terms, nterms, nullptr, &w, &f,
                        &filter);
  if (rc != BG_OK) return rc;
  return join_mark((BgNlJoin*)handle, w, filter);
}

extern "C" int bg_nljoin_build_rows(void* handle, int32_t matched,
                                    int64_t* out_count,
                                    uint32_t* d_out_build) {
  REQUIRE_INIT();
  return join_build_rows((BgNlJoin*)handle, matched, out_count, d_out_build);
}

// sentinel handling for probe-outer joins: split an index vector carrying
// BG_JOIN_NULL_IDX markers into a clamped (safe-to-gather) vector + an
// Arrow validity bitmap of the non-sentinel slots
__global__ void k_idx_sentinel(const uint32_t* __restrict__ idx, int64_t m,
                               uint32_t* __restrict__ clamped,
                               uint32_t* __restrict__ valid_words) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t v = idx[i];
    const bool ok = v != 0xFFFFFFFFu;
    clamped[i] = ok ? v : 0;
    if (ok) atomicOr(&valid_words[i >> 5], 1u << (i & 31));
    else atomicAnd(&valid_words[i >> 5], ~(1u << (i & 31)));
  }
}

extern "C" int bg_idx_sentinel(const uint32_t* d_idx, int64_t m,
                               uint32_t* d_clamped, uint8_t* d_valid_bits) {
  REQUIRE_INIT();
  if (m <= 0) return BG_OK;
  int blocks = (int)bg_imin64((m + BG_BLOCK - 1) / BG_BLOCK, BG_MAX_BLOCKS);
  hipLaunchKernelGGL(k_idx_sentinel, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     d_idx, m, d_clamped, (uint32_t*)d_valid_bits);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

__global__ void k_bitmap_and(const uint8_t* __restrict__ a,
                             const uint8_t* __restrict__ b, int64_t nbytes,
                             uint8_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nbytes;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = a[i] & b[i];
}

extern "C" int bg_bitmap_and(const uint8_t* d_a, const uint8_t* d_b,
                             int64_t nbits, uint8_t* d_out) {
  REQUIRE_INIT();
  int64_t nbytes = (nbits + 7) / 8;
  if (nbytes <= 0) return BG_OK;
  int blocks =
      (int)bg_imin64((nbytes + BG_BLOCK - 1) / BG_BLOCK, BG_MAX_BLOCKS);
  hipLaunchKernelGGL(k_bitmap_and, dim3(blocks), dim3(BG_BLOCK), 0, 0, d_a,
                     d_b, nbytes, d_out);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---------------------------------------------------------------------------
// LIKE predicates over Utf8 columns (FilterExec breadth for the
// q9/q13/q14/q16 shapes: '%green%', 'PROMO%', '%BRASS',
// '%special%requests%').  Pattern restated as up to 4 literal TERMS that
// must appear in order, with anchors: prefix (pattern does not start with
// %) pins term 0 at position 0; suffix (does not end with %) pins the
// last term at the end.  This covers every LIKE in the reference's
// approved/q*.txt plans (no '_' wildcards there).  Output mask ANDs into
// an Arrow bitmap like bg_eval_predicates; NULL input => false.
// ---------------------------------------------------------------------------
#define BG_LIKE_MAX_TERMS 4
#define BG_LIKE_MAX_PAT 64

struct BgLikeArgs {
  const uint8_t* d_data;
  const int32_t* d_offsets;
  const uint8_t* d_validity;
  uint8_t terms[BG_LIKE_MAX_TERMS][BG_LIKE_MAX_PAT];
  int32_t term_len[BG_LIKE_MAX_TERMS];
  int32_t nterms;
  int32_t anchor_prefix, anchor_suffix;
  int32_t negate;  // NOT LIKE
};

__device__ __forceinline__ bool bg_like_row(const BgLikeArgs& a,
                                            const uint8_t* s, int32_t len) {
  int32_t pos = 0;
  for (int t = 0; t < a.nterms; ++t) {
    const int32_t tl = a.term_len[t];
    const bool first = t == 0, last = t == a.nterms - 1;
    if (first && a.anchor_prefix) {
      if (len < tl) return false;
      for (int32_t j = 0; j < tl; ++j)
        if (s[j] != a.terms[t][j]) return false;
      pos = tl;
      if (last && a.anchor_suffix) return len == tl;
      continue;
    }
    if (last && a.anchor_suffix) {
      if (len - pos < tl) return false;
      for (int32_t j = 0; j < tl; ++j)
        if (s[len - tl + j] != a.terms[t][j]) return false;
      return true;
    }
    // find the term anywhere at/after pos
    bool found = false;
    for (int32_t i = pos; i + tl <= len; ++i) {
      bool m = true;
      for (int32_t j = 0; j < tl; ++j)
        if (s[i + j] != a.terms[t][j]) { m = false; break; }
      if (m) { pos = i + tl; found = true; break; }
    }
    if (!found) return false;
  }
  return true;
}

__global__ void k_eval_like(BgLikeArgs a, int64_t n, u64* mask_words) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  const int lane = lane_id();
  const int64_t nwords = (n + 63) / 64;
  for (int64_t w = wave_global; w < nwords; w += nwaves) {
    const int64_t i = w * BG_WAVE + lane;
    bool hit = false;
    if (i < n && bit_valid(a.d_validity, i)) {
      const int32_t lo = a.d_offsets[i], hi = a.d_offsets[i + 1];
      hit = bg_like_row(a, a.d_data + lo, hi - lo);
      if (a.negate) hit = !hit;
    }
    const u64 m = __ballot(hit);
    if (lane == 0) mask_words[w] &= m;  // AND-fold like bg_eval_predicates
  }
}

/* AND a LIKE predicate over a Utf8 column into an EXISTING Arrow LSB
 * bitmask (initialise the mask to all-ones or with bg_eval_predicates
 * first).  terms/lens describe the in-order literal fragments of the
 * pattern; anchors pin the first fragment at the start (no leading %)
 * and/or the last at the end (no trailing %).  negate = NOT LIKE. */
extern "C" int bg_eval_like(const bg_column* col, const char* const* terms,
                            const int32_t* term_lens, int32_t nterms,
                            int32_t anchor_prefix, int32_t anchor_suffix,
                            int32_t negate, int64_t n, uint8_t* d_mask) {
  REQUIRE_INIT();
  if (col->dtype != BG_DT_UTF8 || !col->d_offsets)
    return set_err(BG_ERR_INVALID, "bg_eval_like: Utf8 column required");
  if (nterms < 1 || nterms > BG_LIKE_MAX_TERMS)
    return set_err(BG_ERR_INVALID, "bg_eval_like: 1..4 pattern terms");
  BgLikeArgs a{};
  a.d_data = (const uint8_t*)col->d_data;
  a.d_offsets = col->d_offsets;
  a.d_validity = col->d_validity;
  a.nterms = nterms;
  a.anchor_prefix = anchor_prefix;
  a.anchor_suffix = anchor_suffix;
  a.negate = negate;
  for (int t = 0; t < nterms; ++t) {
    if (term_lens[t] <= 0 || term_lens[t] > BG_LIKE_MAX_PAT)
      return set_err(BG_ERR_INVALID, "bg_eval_like: term length 1..64");
    a.term_len[t] = term_lens[t];
    memcpy(a.terms[t], terms[t], (size_t)term_lens[t]);
  }
  const int64_t nwords = (n + 63) / 64;
  int blocks = grid_for(nwords * BG_WAVE);
  hipLaunchKernelGGL(k_eval_like, dim3(blocks), dim3(BG_BLOCK), 0, 0, a, n,
                     (u64*)d_mask);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// CASE WHEN <pred> THEN a ELSE b (ProjectionExec breadth: q8/q12/q14-class
// conditional expressions): elementwise select through an Arrow bitmask.
__global__ void k_select(const u64* __restrict__ mask,
                         const uint8_t* __restrict__ a,
                         const uint8_t* __restrict__ b, int64_t esz,
                         int64_t n, uint8_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const bool sel = (mask[i >> 6] >> (i & 63)) & 1;
    const uint8_t* src = (sel ? a : b) + i * esz;
    uint8_t* dst = out + i * esz;
    for (int64_t j = 0; j < esz; ++j) dst[j] = src[j];
  }
}

extern "C" int bg_select(const uint8_t* d_mask, const void* d_a,
                         const void* d_b, int64_t esz, int64_t n,
                         void* d_out) {
  REQUIRE_INIT();
  if (n <= 0) return BG_OK;
  int blocks = (int)bg_imin64((n + BG_BLOCK - 1) / BG_BLOCK, BG_MAX_BLOCKS);
  hipLaunchKernelGGL(k_select, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (const u64*)d_mask, (const uint8_t*)d_a,
                     (const uint8_t*)d_b, esz, n, (uint8_t*)d_out);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// constant fill (literal branches of CASE, constant columns)
__global__ void k_fill_const(uint8_t* __restrict__ out, int64_t n,
                             int64_t esz, int64_t lo, int64_t hi) {
  const uint8_t v[16] = {
      (uint8_t)(lo), (uint8_t)(lo >> 8), (uint8_t)(lo >> 16),
      (uint8_t)(lo >> 24), (uint8_t)(lo >> 32), (uint8_t)(lo >> 40),
      (uint8_t)(lo >> 48), (uint8_t)(lo >> 56), (uint8_t)(hi),
      (uint8_t)(hi >> 8), (uint8_t)(hi >> 16), (uint8_t)(hi >> 24),
      (uint8_t)(hi >> 32), (uint8_t)(hi >> 40), (uint8_t)(hi >> 48),
      (uint8_t)(hi >> 56)};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint8_t* dst = out + i * esz;
    for (int64_t j = 0; j < esz; ++j) dst[j] = v[j];
  }
}

extern "C" int bg_fill_const(void* d_out, int64_t n, int64_t esz,
                             int64_t lo, int64_t hi) {
  REQUIRE_INIT();
  if (n <= 0) return BG_OK;
  if (esz <= 0 || esz > 16)
    return set_err(BG_ERR_INVALID, "bg_fill_const: esz 1..16");
  int blocks = (int)bg_imin64((n + BG_BLOCK - 1) / BG_BLOCK, BG_MAX_BLOCKS);
  hipLaunchKernelGGL(k_fill_const, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (uint8_t*)d_out, n, esz, lo, hi);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// IN-list predicate (q12 l_shipmode IN (...), q19 p_container IN (...)):
// AND-fold `x IN {v0..vk}` over an integer/dict column into an existing
// Arrow bitmask.  k <= 16 values, compared as i64 (narrower dtypes
// sign-extend; dict8 zero-extends).
__global__ void k_eval_in(const uint8_t* __restrict__ data,
                          const uint8_t* __restrict__ valid, int32_t dtype,
                          const int64_t* __restrict__ vals, int32_t nvals,
                          int64_t n, u64* __restrict__ mask_words) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  const int lane = lane_id();
  const int64_t nwords = (n + 63) / 64;
  for (int64_t w = wave_global; w < nwords; w += nwaves) {
    const int64_t i = w * BG_WAVE + lane;
    bool hit = false;
    if (i < n && bit_valid(valid, i)) {
      int64_t x;
      switch (dtype) {
        case BG_DT_INT64: x = reinterpret_cast<const int64_t*>(data)[i]; break;
        case BG_DT_INT32:
        case BG_DT_DATE32: x = reinterpret_cast<const int32_t*>(data)[i]; break;
        case BG_DT_DICT8: x = data[i]; break;
        default: x = 0;
      }
      for (int v = 0; v < nvals; ++v)
        if (vals[v] == x) { hit = true; break; }
    }
    const u64 m = __ballot(hit);
    if (lane == 0) mask_words[w] &= m;
  }
}

extern "C" int bg_eval_in(const bg_column* col, const int64_t* values,
                          int32_t nvalues, int64_t n, uint8_t* d_mask) {
  REQUIRE_INIT();
  if (nvalues < 1 || nvalues > 16)
    return set_err(BG_ERR_INVALID, "bg_eval_in: 1..16 values");
  if (col->dtype != BG_DT_INT64 && col->dtype != BG_DT_INT32 &&
      col->dtype != BG_DT_DATE32 && col->dtype != BG_DT_DICT8)
    return set_err(BG_ERR_UNSUPPORTED, "bg_eval_in: integer/dict column");
  DevBuf<int64_t> d_vals;
  HIP_TRY(d_vals.alloc(16));
  HIP_TRY(hipMemcpy(d_vals, values, sizeof(int64_t) * nvalues,
                    hipMemcpyHostToDevice));
  const int64_t nwords = (n + 63) / 64;
  int blocks = grid_for(nwords * BG_WAVE);
  hipLaunchKernelGGL(k_eval_in, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     (const uint8_t*)col->d_data, col->d_validity,
                     col->dtype, d_vals, nvalues, n, (u64*)d_mask);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

__global__ void k_bitmap_or(const uint8_t* __restrict__ a,
                            const uint8_t* __restrict__ b, int64_t nbytes,
                            uint8_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nbytes;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = a[i] | b[i];
}

extern "C" int bg_bitmap_or(const uint8_t* d_a, const uint8_t* d_b,
                            int64_t nbits, uint8_t* d_out) {
  REQUIRE_INIT();
  int64_t nbytes = (nbits + 7) / 8;
  if (nbytes <= 0) return BG_OK;
  int blocks =
      (int)bg_imin64((nbytes + BG_BLOCK - 1) / BG_BLOCK, BG_MAX_BLOCKS);
  hipLaunchKernelGGL(k_bitmap_or, dim3(blocks), dim3(BG_BLOCK), 0, 0, d_a,
                     d_b, nbytes, d_out);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Scalar expressions of the approved plans that are neither Decimal128
// arithmetic nor a column-vs-literal predicate: date_part (q7/q8/q9),
// substr and Utf8 IN-lists (q22), column-vs-column compares (q4/q12/q21).
// ---------------------------------------------------------------------------

// One Date32 day number -> one date part, proleptic Gregorian, exact for
// EVERY int32 input in 32-bit arithmetic.  The civil-from-days chain wants
// z + 719468 (days since 0000-03-01) floor-divided by the 146097-day era;
// with u = z + 2^31 (u32, a sign-bit flip) that is
//   z + 719468 = (u - 14862) - 14694 * 146097,
// so u - 14862 divides unsigned.  Only the lowest 14862 inputs would wrap:
// they take one era more (u + 131235 < 146097) and era - 1 instead.  No
// signed value ever leaves [-5.9M, 5.9M]; every division is u32 by a
// constant.
template <int PART>
__device__ __forceinline__ int32_t date_part_one(int32_t z) {
  const uint32_t u = (uint32_t)z ^ 0x80000000u;
  if (PART == BG_DATE_PART_DOW) {
    // 1970-01-01 is a Thursday (4) and 2^31 mod 7 == 2: dow = (u - 2 + 4) % 7
    const uint32_t r = u % 7u + 2u;
    return (int32_t)(r >= 7u ? r - 7u : r);
  }
  const bool low = u < 14862u;
  const uint32_t v = low ? u + 131235u : u - 14862u;
  const uint32_t e = v / 146097u;
  const uint32_t doe = v - e * 146097u;                          // [0, 146096]
  const uint32_t yoe =
      (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u; // [0, 399]
  const uint32_t doy =
      doe - (365u * yoe + yoe / 4u - yoe / 100u);                // [0, 365]
  const uint32_t mp = (5u * doy + 2u) / 153u;                    // [0, 11]
  const bool jan_feb = mp >= 10u;  // the March-based year's last two months
  if (PART == BG_DATE_PART_DAY)
    return (int32_t)(doy - (153u * mp + 2u) / 5u + 1u);
  if (PART == BG_DATE_PART_DOY) {
    if (jan_feb) return (int32_t)(doy - 305u);  // Jan 1 is March-based day 306
    const bool leap = (yoe & 3u) == 0u && (yoe % 100u != 0u || yoe == 0u);
    return (int32_t)(doy + 60u + (leap ? 1u : 0u));
  }
  const uint32_t m = jan_feb ? mp - 9u : mp + 3u;                // [1, 12]
  if (PART == BG_DATE_PART_MONTH) return (int32_t)m;
  if (PART == BG_DATE_PART_QUARTER) return (int32_t)((m + 2u) / 3u);
  const int32_t era = (int32_t)e - (low ? 14695 : 14694);
  return (int32_t)yoe + era * 400 + (jan_feb ? 1 : 0);
}

// streaming: 4 B in, 4 B out per row; four rows per lane through 16-byte
// non-temporal accesses (nvec of them), scalar tail for the last n % 4
template <int PART>
__global__ __launch_bounds__(BG_BLOCK) void k_date_part(
    const int32_t* __restrict__ in, int64_t n, int64_t nvec,
    int32_t* __restrict__ out) {
  typedef int i32x4_dp __attribute__((ext_vector_type(4)));
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = tid; v < nvec; v += stride) {
    const i32x4_dp x = __builtin_nontemporal_load(
        reinterpret_cast<const i32x4_dp*>(in) + v);
    i32x4_dp r;
    r[0] = date_part_one<PART>(x[0]);
    r[1] = date_part_one<PART>(x[1]);
    r[2] = date_part_one<PART>(x[2]);
    r[3] = date_part_one<PART>(x[3]);
    __builtin_nontemporal_store(r, reinterpret_cast<i32x4_dp*>(out) + v);
  }
  for (int64_t i = nvec * 4 + tid; i < n; i += stride)
    out[i] = date_part_one<PART>(in[i]);
}

template <int PART>
static void launch_date_part(const int32_t* in, int64_t n, int32_t* out) {
  // the 16-byte path needs both pointers 16-byte aligned (sliced columns
  // may not be); otherwise every row takes the scalar loop
  const bool aligned = (((uintptr_t)in | (uintptr_t)out) & 15u) == 0;
  const int64_t nvec = aligned ? n / 4 : 0;
  const int blocks = grid_for(nvec > 0 ? nvec : n);
  hipLaunchKernelGGL(k_date_part<PART>, dim3(blocks), dim3(BG_BLOCK), 0, 0, in,
                     n, nvec, out);
}

extern "C" int bg_date_part(const bg_column* col, int32_t part, int64_t n,
                            int32_t* d_out) {
  REQUIRE_INIT();
  if (col->dtype != BG_DT_DATE32)
    return set_err(BG_ERR_INVALID, "bg_date_part: Date32 column required");
  if (n < 0) return set_err(BG_ERR_INVALID, "bg_date_part: negative n");
  const int32_t* in = (const int32_t*)col->d_data;
  switch (part) {
    case BG_DATE_PART_YEAR:
      launch_date_part<BG_DATE_PART_YEAR>(in, n, d_out); break;
    case BG_DATE_PART_QUARTER:
      launch_date_part<BG_DATE_PART_QUARTER>(in, n, d_out); break;
    case BG_DATE_PART_MONTH:
      launch_date_part<BG_DATE_PART_MONTH>(in, n, d_out); break;
    case BG_DATE_PART_DAY:
      launch_date_part<BG_DATE_PART_DAY>(in, n, d_out); break;
    case BG_DATE_PART_DOY:
      launch_date_part<BG_DATE_PART_DOY>(in, n, d_out); break;
    case BG_DATE_PART_DOW:
      launch_date_part<BG_DATE_PART_DOW>(in, n, d_out); break;
    default:
      return set_err(BG_ERR_UNSUPPORTED,
                     "bg_date_part: part must be year/quarter/month/day/"
                     "doy/dow");
  }
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// substr bounds pass, one lane per row: walk the row's bytes counting
// code-point starts until code point `e` is reached, remembering where code
// point `s` began.  Emits the slice's byte length and source address — the
// (lens, srcaddr) pair bg_ba_materialize lays out and copies.  s >= 0 and e
// arrive clamped/saturated from the host; NULL rows emit zero bytes and
// read no payload.
__global__ void k_substr_bounds(const uint8_t* __restrict__ data,
                                const int32_t* __restrict__ offs,
                                const uint8_t* __restrict__ valid, int64_t s,
                                int64_t e, int64_t n,
                                int64_t* __restrict__ lens,
                                int64_t* __restrict__ srcaddr) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t len = 0;
    const uint8_t* src = nullptr;
    if (e > s && bit_valid(valid, i)) {
      const int32_t lo = offs[i], hi = offs[i + 1];
      int32_t bs = hi, be = hi;  // row shorter than s / e code points
      int64_t cp = 0;
      for (int32_t b = lo; b < hi; ++b) {
        if ((data[b] & 0xC0) == 0x80) continue;  // continuation byte
        if (cp == s) bs = b;
        if (cp == e) { be = b; break; }
        ++cp;
      }
      len = be - bs;
      if (len > 0) src = data + bs;
    }
    lens[i] = len;
    srcaddr[i] = (int64_t)(uintptr_t)src;
  }
}

extern "C" int bg_substr(const bg_column* col, int64_t start,
                         int32_t has_count, int64_t count, int64_t n,
                         int32_t* d_out_offsets, void* d_out_data,
                         int64_t out_data_cap, int64_t* out_total_bytes) {
  REQUIRE_INIT();
  if (col->dtype != BG_DT_UTF8 || !col->d_offsets)
    return set_err(BG_ERR_INVALID, "bg_substr: Utf8 column required");
  if (has_count && count < 0)
    return set_err(BG_ERR_INVALID,
                   "bg_substr: negative substring length not allowed");
  if (n < 0) return set_err(BG_ERR_INVALID, "bg_substr: negative n");
  // code points [max(s, 0), e) with s = start - 1, e = s + count; both
  // saturate instead of wrapping (a row never holds 2^63 code points)
  const int64_t s0 = start == INT64_MIN ? INT64_MIN : start - 1;
  int64_t e = INT64_MAX;  // no count: to the end of the row
  if (has_count && __builtin_add_overflow(s0, count, &e))
    e = INT64_MAX;  // count >= 0: the sum can only overflow upwards
  const int64_t s = s0 < 0 ? 0 : s0;
  DevBuf<int64_t> d_lens;
  DevBuf<int64_t> d_srcaddr;
  HIP_TRY(d_lens.alloc(n));
  HIP_TRY(d_srcaddr.alloc(n));
  hipLaunchKernelGGL(k_substr_bounds, dim3(grid_for(n)), dim3(BG_BLOCK), 0, 0,
                     (const uint8_t*)col->d_data, col->d_offsets,
                     col->d_validity, s, e, n, d_lens.get(), d_srcaddr.get());
  HIP_TRY(hipGetLastError());
  // layout + copy (and the d_out_data == NULL sizing convention) are
  // bg_ba_materialize's
  int rc = bg_ba_materialize(d_lens, d_srcaddr, n, d_out_offsets,
                             (uint8_t*)d_out_data, out_data_cap,
                             out_total_bytes);
  if (rc != BG_OK) return rc;
  if (*out_total_bytes > 0x7fffffffLL)
    return set_err(BG_ERR_INVALID, "bg_substr: >2GiB Utf8 result");
  return BG_OK;
}

// Column-vs-column compare (q4/q12/q21: l_receiptdate > l_commitdate,
// l_shipdate < l_commitdate).  As k_eval_predicates, one wave per 64 rows
// and ballot word == bitmap word, but it reads the mask word FIRST: a wave
// whose word is already zero loads neither column (after q12's literal date
// window about one row in seven is left), and a lane whose bit is clear
// loads nothing.  Stores old & ballot; rows >= n never vote, so the last
// word's tail bits come out 0.
template <typename T>
__device__ __forceinline__ T cmp_load(const void* base, int64_t row) {
  return __builtin_nontemporal_load(reinterpret_cast<const T*>(base) + row);
}
// Decimal128 as signed i128: high word signed, low word unsigned
template <>
__device__ __forceinline__ i128 cmp_load<i128>(const void* base, int64_t row) {
  typedef unsigned long long ull2_cc __attribute__((ext_vector_type(2)));
  const ull2_cc v = __builtin_nontemporal_load(
      reinterpret_cast<const ull2_cc*>(base) + row);
  return make_i128(v[0], (i64)v[1]);
}

template <typename T>
__global__ void k_eval_compare_cols(const void* __restrict__ a,
                                    const uint8_t* __restrict__ avalid,
                                    const void* __restrict__ b,
                                    const uint8_t* __restrict__ bvalid,
                                    int cmp, int64_t n, u64* mask_words,
                                    int64_t nwords) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  const int lane = lane_id();
  for (int64_t w = wave_global; w < nwords; w += nwaves) {
    const u64 old = mask_words[w];
    if (old == 0) continue;  // wave-uniform: nothing left to decide
    const int64_t row = w * BG_WAVE + lane;
    bool keep = row < n && ((old >> lane) & 1) && bit_valid(avalid, row) &&
                bit_valid(bvalid, row);
    if (keep) {
      const T x = cmp_load<T>(a, row), y = cmp_load<T>(b, row);
      switch (cmp) {
        case BG_CMP_LT: keep = x < y; break;
        case BG_CMP_LE: keep = x <= y; break;
        case BG_CMP_GT: keep = x > y; break;
        case BG_CMP_GE: keep = x >= y; break;
        case BG_CMP_EQ: keep = x == y; break;
        default: keep = x != y; break;  // BG_CMP_NE (host checked the range)
      }
    }
    const u64 m = __ballot(keep);
    if (lane == 0) mask_words[w] = old & m;
  }
}

extern "C" int bg_eval_compare_cols(const bg_column* a, const bg_column* b,
                                    int32_t cmp, int64_t n, uint8_t* d_mask) {
  REQUIRE_INIT();
  if (cmp < BG_CMP_LT || cmp > BG_CMP_NE)
    return set_err(BG_ERR_INVALID, "bg_eval_compare_cols: unknown cmp");
  if (a->dtype == BG_DT_FLOAT64 || a->dtype == BG_DT_UTF8 ||
      b->dtype == BG_DT_FLOAT64 || b->dtype == BG_DT_UTF8)
    return set_err(BG_ERR_UNSUPPORTED,
                   "bg_eval_compare_cols: Float64/Utf8 columns");
  if (a->dtype != b->dtype)
    return set_err(BG_ERR_INVALID, "bg_eval_compare_cols: dtype mismatch");
  if (a->dtype == BG_DT_DECIMAL128 && a->scale != b->scale)
    return set_err(BG_ERR_INVALID,
                   "bg_eval_compare_cols: Decimal128 scale mismatch");
  if (n < 0) return set_err(BG_ERR_INVALID, "bg_eval_compare_cols: negative n");
  const int64_t nwords = (n + 63) / 64;
  const int blocks = grid_for(nwords * BG_WAVE);
#define BG_LAUNCH_CMP(T)                                                      \
  hipLaunchKernelGGL(k_eval_compare_cols<T>, dim3(blocks), dim3(BG_BLOCK), 0, \
                     0, a->d_data, a->d_validity, b->d_data, b->d_validity,   \
                     cmp, n, (u64*)d_mask, nwords)
  switch (a->dtype) {
    case BG_DT_INT32:
    case BG_DT_DATE32: BG_LAUNCH_CMP(int32_t); break;
    case BG_DT_INT64: BG_LAUNCH_CMP(int64_t); break;
    case BG_DT_DICT8: BG_LAUNCH_CMP(uint8_t); break;
    case BG_DT_DECIMAL128: BG_LAUNCH_CMP(i128); break;
    default:
      return set_err(BG_ERR_INVALID, "bg_eval_compare_cols: unknown dtype");
  }
#undef BG_LAUNCH_CMP
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// Utf8 IN-list (q22: substr(c_phone, 1, 2) IN ('13', '31', ...)): exact
// byte equality against up to 16 literals of up to 64 bytes, passed by
// value like BgLikeArgs.  ANDs into the mask; NULL => false.
#define BG_IN_UTF8_MAX_VALUES 16

struct BgInUtf8Args {
  const uint8_t* d_data;
  const int32_t* d_offsets;
  const uint8_t* d_validity;
  uint8_t vals[BG_IN_UTF8_MAX_VALUES][BG_LIKE_MAX_PAT];
  int32_t val_len[BG_IN_UTF8_MAX_VALUES];
  int32_t nvals;
};

__global__ void k_eval_in_utf8(BgInUtf8Args a, int64_t n, u64* mask_words) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  const int lane = lane_id();
  const int64_t nwords = (n + 63) / 64;
  for (int64_t w = wave_global; w < nwords; w += nwaves) {
    const int64_t i = w * BG_WAVE + lane;
    bool hit = false;
    if (i < n && bit_valid(a.d_validity, i)) {
      const int32_t lo = a.d_offsets[i], len = a.d_offsets[i + 1] - lo;
      const uint8_t* s = a.d_data + lo;
      for (int v = 0; v < a.nvals && !hit; ++v) {
        if (a.val_len[v] != len) continue;
        bool eq = true;
        for (int32_t j = 0; j < len; ++j)
          if (s[j] != a.vals[v][j]) { eq = false; break; }
        hit = eq;
      }
    }
    const u64 m = __ballot(hit);
    if (lane == 0) mask_words[w] &= m;
  }
}

extern "C" int bg_eval_in_utf8(const bg_column* col, const char* const* values,
                               const int32_t* value_lens, int32_t nvalues,
                               int64_t n, uint8_t* d_mask) {
  REQUIRE_INIT();
  if (col->dtype != BG_DT_UTF8 || !col->d_offsets)
    return set_err(BG_ERR_INVALID, "bg_eval_in_utf8: Utf8 column required");
  if (nvalues < 1 || nvalues > BG_IN_UTF8_MAX_VALUES)
    return set_err(BG_ERR_INVALID, "bg_eval_in_utf8: 1..16 values");
  if (n < 0) return set_err(BG_ERR_INVALID, "bg_eval_in_utf8: negative n");
  BgInUtf8Args a{};
  a.d_data = (const uint8_t*)col->d_data;
  a.d_offsets = col->d_offsets;
  a.d_validity = col->d_validity;
  a.nvals = nvalues;
  for (int v = 0; v < nvalues; ++v) {
    if (value_lens[v] <= 0 || value_lens[v] > BG_LIKE_MAX_PAT)
      return set_err(BG_ERR_INVALID, "bg_eval_in_utf8: value length 1..64");
    a.val_len[v] = value_lens[v];
    memcpy(a.vals[v], values[v], (size_t)value_lens[v]);
  }
  const int64_t nwords = (n + 63) / 64;
  int blocks = grid_for(nwords * BG_WAVE);
  hipLaunchKernelGGL(k_eval_in_utf8, dim3(blocks), dim3(BG_BLOCK), 0, 0, a, n,
                     (u64*)d_mask);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Multi-expression Decimal128 projection in ONE pass (round 2): q1-class
// stages evaluate several arithmetic expressions over the same columns;
// chaining bg_project_dec128 launches materialises every intermediate
// (q1: ~77 GB of extra HBM traffic at SF100).  This kernel interprets a
// tiny stack bytecode per row — each input column is read once, each
// output written once, intermediates live in registers.
// ---------------------------------------------------------------------------
#define BG_EXPR_PUSH_COL 0 /* arg = column index */
#define BG_EXPR_PUSH_LIT 1 /* arg = literal index */
#define BG_EXPR_MUL 2
#define BG_EXPR_ADD 3
#define BG_EXPR_SUB 4      /* top = below - top */
#define BG_EXPR_MAX_OPS 24
#define BG_EXPR_MAX_OUT 6
#define BG_EXPR_MAX_LITS 8

struct BgExprProg {
  int32_t ops[BG_EXPR_MAX_OPS];
  int32_t args[BG_EXPR_MAX_OPS];
  int32_t nops;
  int32_t expr_end[BG_EXPR_MAX_OUT];  // bytecode index AFTER each expr
  int32_t nexprs;
  i64 lit_lo[BG_EXPR_MAX_LITS];
  i64 lit_hi[BG_EXPR_MAX_LITS];
  const void* col_data[BG_MAX_AGGS];
  int32_t col_dtype[BG_MAX_AGGS];
  int32_t ncols;
  void* out[BG_EXPR_MAX_OUT];
};

// The obvious interpreter (i128 stack[5], BgExprProg by value, dynamic
// indexing everywhere) allocates 648 B of scratch per lane — every
// PUSH/POP is an HBM round-trip and q1 at SF100 ran 60.5ms -> 272ms.
// Two constraints recover a register-only kernel: (1) the program lives
// in device memory, so ops[k]/col_data[c] are uniform cached loads, not
// a scratch copy of the kernarg struct; (2) the value stack is five
// explicit i128 registers selected by switches on sp — sp is uniform
// across the wavefront (all lanes run the same bytecode), so the
// switches cost branches, never divergence or scratch.
__global__ void k_project_multi(const BgExprProg* __restrict__ pp,
                                int64_t n) {
  const BgExprProg& p = *pp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    i128 s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    int sp = 0;
    int e = 0;
    for (int k = 0; k < p.nops; ++k) {
      const int op = p.ops[k];
      if (op == BG_EXPR_PUSH_COL || op == BG_EXPR_PUSH_LIT) {
        i128 v;
        if (op == BG_EXPR_PUSH_COL) {
          const int c = p.args[k];
          if (p.col_dtype[c] == BG_DT_DECIMAL128) {
            const ulong2 w =
                reinterpret_cast<const ulong2*>(p.col_data[c])[i];
            v = make_i128(w.x, (i64)w.y);
          } else {
            v = (i128) reinterpret_cast<const int64_t*>(p.col_data[c])[i];
          }
        } else {
          v = make_i128((u64)p.lit_lo[p.args[k]], p.lit_hi[p.args[k]]);
        }
        switch (sp) {
          case 0: s0 = v; break;
          case 1: s1 = v; break;
          case 2: s2 = v; break;
          case 3: s3 = v; break;
          default: s4 = v; break;
        }
        ++sp;
      } else {
        // binary op on (below, top): result replaces the pair
        switch (sp) {
          case 2:
            s0 = (op == BG_EXPR_MUL)   ? s0 * s1
                 : (op == BG_EXPR_ADD) ? s0 + s1
                                       : s0 - s1;
            break;
          case 3:
            s1 = (op == BG_EXPR_MUL)   ? s1 * s2
                 : (op == BG_EXPR_ADD) ? s1 + s2
                                       : s1 - s2;
            break;
          case 4:
            s2 = (op == BG_EXPR_MUL)   ? s2 * s3
                 : (op == BG_EXPR_ADD) ? s2 + s3
                                       : s2 - s3;
            break;
          default:
            s3 = (op == BG_EXPR_MUL)   ? s3 * s4
                 : (op == BG_EXPR_ADD) ? s3 + s4
                                       : s3 - s4;
            break;
        }
        --sp;
      }
      if (k + 1 == p.expr_end[e]) {
        --sp;
        i128 v;
        switch (sp) {
          case 0: v = s0; break;
          case 1: v = s1; break;
          case 2: v = s2; break;
          case 3: v = s3; break;
          default: v = s4; break;
        }
        ulong2* o = reinterpret_cast<ulong2*>(p.out[e]);
        ulong2 w;
        w.x = (u64)(u128)v;
        w.y = (u64)((u128)v >> 64);
        o[i] = w;
        ++e;
      }
    }
  }
}

extern "C" int bg_project_dec128_multi(
    const bg_column* cols, int32_t ncols, const int32_t* ops,
    const int32_t* args, int32_t nops, const int32_t* expr_end,
    int32_t nexprs, const int64_t* lit_lo, const int64_t* lit_hi,
    int32_t nlits, int64_t n, void* const* d_outs) {
  REQUIRE_INIT();
  if (ncols < 0 || ncols > BG_MAX_AGGS || nops < 1 ||
      nops > BG_EXPR_MAX_OPS || nexprs < 1 || nexprs > BG_EXPR_MAX_OUT ||
      nlits < 0 || nlits > BG_EXPR_MAX_LITS)
    return set_err(BG_ERR_INVALID, "bg_project_dec128_multi: limits");
  BgExprProg p{};
  p.nops = nops;
  p.nexprs = nexprs;
  p.ncols = ncols;
  for (int k = 0; k < nops; ++k) {
    p.ops[k] = ops[k];
    p.args[k] = args[k];
  }
  for (int e = 0; e < nexprs; ++e) {
    p.expr_end[e] = expr_end[e];
    p.out[e] = d_outs[e];
  }
  for (int l = 0; l < nlits; ++l) {
    p.lit_lo[l] = lit_lo[l];
    p.lit_hi[l] = lit_hi[l];
  }
  for (int c = 0; c < ncols; ++c) {
    p.col_data[c] = cols[c].d_data;
    p.col_dtype[c] = cols[c].dtype;
    if (cols[c].dtype != BG_DT_DECIMAL128 && cols[c].dtype != BG_DT_INT64)
      return set_err(BG_ERR_UNSUPPORTED,
                     "bg_project_dec128_multi: dec128/int64 inputs");
  }
  DevBuf<BgExprProg> d_p;
  HIP_TRY(d_p.alloc(1));
  HIP_TRY(hipMemcpy(d_p, &p, sizeof(BgExprProg), hipMemcpyHostToDevice));
  int blocks = grid_for(n);
  hipLaunchKernelGGL(k_project_multi, dim3(blocks), dim3(BG_BLOCK), 0, 0,
                     d_p, n);
  int rc = hipGetLastError() == hipSuccess ? BG_OK : BG_ERR_HIP;
  if (rc != BG_OK) return set_err(BG_ERR_HIP, "k_project_multi launch");
  return BG_OK;
}

// ---------------------------------------------------------------------------
// CAST, Float64 arithmetic and Decimal128 division (approved/q8.txt:103,
// q11.txt:70,74, q14.txt:22, q17.txt:19,27,33, q20.txt:49, q22.txt:18).
// Elementwise, one row per lane.  A conversion that can fail on a row
// (DataFusion casts with safe=false, decimal div raises DivideByZero) runs
// through k_rows_checked: whole waves walk 64-row words, NULL rows are
// never examined, failing VALID rows are counted by ballot + popcount and
// each wave that saw one adds its count with a single atomic.  A
// conversion that cannot fail runs through k_rows: no counter, no read
// back.
// ---------------------------------------------------------------------------

// One 64-row word of an Arrow validity bitmap of which only ceil(n/8) bytes
// are known to exist: an 8-byte load where the whole word lies inside them
// and the bitmap is 8-byte aligned, the remaining bytes one by one else.
__device__ __forceinline__ u64 valid_word(const uint8_t* bm, int64_t w,
                                          int64_t n) {
  const int64_t nbytes = (n + 7) >> 3, off = w << 3;
  if (((uintptr_t)bm & 7u) == 0 && off + 8 <= nbytes)
    return *reinterpret_cast<const u64*>(bm + off);
  u64 v = 0;
  for (int k = 0; k < 8 && off + k < nbytes; ++k)
    v |= (u64)bm[off + k] << (8 * k);
  return v;
}

__device__ __forceinline__ void store_dec128(void* base, int64_t row, i128 v) {
  ulong2 o;
  o.x = (u64)(u128)v;
  o.y = (u64)((u128)v >> 64);
  reinterpret_cast<ulong2*>(base)[row] = o;
}

__device__ __forceinline__ u128 abs_u128(i128 x) {
  return x < 0 ? (u128)0 - (u128)x : (u128)x;
}

__device__ __forceinline__ i128 signed_i128(u128 mag, bool neg) {
  return (i128)(neg ? (u128)0 - mag : mag);
}

// (double)x of an i128, rounded once to nearest-even: the magnitude's top
// 64 bits with every dropped bit folded into bit 0 (far below the round
// bit at bit 10) convert with the single rounding of u64 -> f64, and the
// power-of-two scale is exact.
__device__ __forceinline__ double i128_to_f64(i128 x) {
  const u128 u = abs_u128(x);
  const u64 hi = (u64)(u >> 64), lo = (u64)u;
  double r;
  if (hi == 0) {
    r = (double)lo;
  } else {
    const int lz = __clzll((long long)hi);
    const u64 top = lz ? (hi << lz) | (lo >> (64 - lz)) : hi;
    const u64 dropped = lz ? lo << lz : lo;
    r = ldexp((double)(top | (u64)(dropped != 0)), 64 - lz);
  }
  return x < 0 ? -r : r;
}

// an INTEGRAL double of magnitude below 2^127 as i128, exactly
__device__ __forceinline__ i128 f64_integral_to_i128(double r) {
  const u64 bits = (u64)__double_as_longlong(r);
  const int e = (int)((bits >> 52) & 0x7FF);
  if (e < 1023) return 0;  // |r| < 1
  const u64 m = (bits & 0xFFFFFFFFFFFFFull) | (1ull << 52);
  const int sh = e - 1075;  // |r| = m * 2^sh, sh <= 74
  const u128 u = sh >= 0 ? (u128)m << sh : (u128)(m >> -sh);
  return signed_i128(u, (bits >> 63) != 0);
}

// Each row functor's run(row) loads, converts, stores and returns 0, or
// the 1-based kind of failure the row met.
template <typename Op>
__global__ __launch_bounds__(BG_BLOCK) void k_rows(Op op, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    (void)op.run(i);
}

// failed[k-1] += number of valid rows whose run() returned k (1..KINDS)
template <int KINDS, typename Op>
__global__ __launch_bounds__(BG_BLOCK) void k_rows_checked(
    Op op, const uint8_t* __restrict__ avalid,
    const uint8_t* __restrict__ bvalid, int64_t n, u64* failed) {
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  u64 nfail[KINDS] = {};
  // the wave's first row: a multiple of 64, so one bitmap word per step
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane;
       base < n; base += stride) {
    u64 live = ~0ull;
    if (avalid) live &= valid_word(avalid, base >> 6, n);
    if (bvalid) live &= valid_word(bvalid, base >> 6, n);
    const int64_t row = base + lane;
    int fail = 0;
    if (row < n && ((live >> lane) & 1)) fail = op.run(row);
#pragma unroll
    for (int k = 0; k < KINDS; ++k)
      nfail[k] += (u64)__popcll(__ballot(fail == k + 1));
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < KINDS; ++k)
      if (nfail[k]) atomicAdd(&failed[k], nfail[k]);
  }
}

template <typename S>
__device__ __forceinline__ i128 load_as_i128(const void* base, int64_t row) {
  if constexpr (sizeof(S) == 16)
    return load_dec128(base, row);
  else
    return (i128) reinterpret_cast<const S*>(base)[row];
}

// Int32 / Int64 -> Float64: (double)x.  Decimal128(p,s) -> Float64:
// (double)x / 1e<s>, two correctly rounded operations.
template <typename S>
struct OpCastToF64 {
  const void* in;
  double p10;
  double* out;
  __device__ __forceinline__ int run(int64_t i) const {
    if constexpr (sizeof(S) == 16)
      out[i] = i128_to_f64(load_dec128(in, i)) / p10;
    else
      out[i] = (double)reinterpret_cast<const S*>(in)[i];
    return 0;
  }
};

struct OpCastI32ToI64 {
  const int32_t* in;
  int64_t* out;
  __device__ __forceinline__ int run(int64_t i) const {
    out[i] = (int64_t)in[i];
    return 0;
  }
};

// x * 10^k into Decimal128(p,s); fails where |x| >= bound = 10^(p-k), which
// is |x * 10^k| >= 10^p without a multiply that could wrap
template <typename S>
struct OpCastScaleUp {
  const void* in;
  i128 mul;
  u128 bound;
  void* out;
  __device__ __forceinline__ int run(int64_t i) const {
    const i128 x = load_as_i128<S>(in, i);
    store_dec128(out, i, (i128)((u128)x * (u128)mul));
    return abs_u128(x) >= bound ? 1 : 0;
  }
};

// x / 10^k rounded half away from zero; fails where |result| >= 10^p
struct OpCastScaleDown {
  const void* in;
  u128 div, limit;
  void* out;
  __device__ __forceinline__ int run(int64_t i) const {
    const i128 x = load_dec128(in, i);
    const u128 u = abs_u128(x);
    u128 q = u / div;
    const u128 r = u - q * div;
    if (2 * r >= div) q += 1;  // r < div <= 10^38: 2 * r cannot wrap
    store_dec128(out, i, signed_i128(q, x < 0));
    return q >= limit ? 1 : 0;
  }
};

// round(v * 1e<s>), C round(); fails on NaN, +-inf and |r| >= 10^p
struct OpCastF64ToDec {
  const double* in;
  double p10;
  u128 limit;
  void* out;
  __device__ __forceinline__ int run(int64_t i) const {
    const double r = round(in[i] * p10);
    // NaN compares false; 2^127 bounds what f64_integral_to_i128 takes
    bool ok = fabs(r) < 1.7014118346046923e38;
    const i128 q = ok ? f64_integral_to_i128(r) : (i128)0;
    ok = ok && abs_u128(q) < limit;
    store_dec128(out, i, ok ? q : (i128)0);
    return ok ? 0 : 1;
  }
};

// arrow-rs decimal div after scale alignment: (a * 10^m) / b for UP, else
// a / (b * 10^m), truncated toward zero.  Kind 1: b == 0.  Kind 2: the
// scaled operand leaves i128 (|operand| > fit = (2^127 - 1) / 10^m).
template <bool UP>
struct OpDivDec128 {
  const void* a;
  const void* b;
  u128 p10, fit;
  void* out;
  __device__ __forceinline__ int run(int64_t i) const {
    const i128 x = load_dec128(a, i), y = load_dec128(b, i);
    u128 ux = abs_u128(x), uy = abs_u128(y);
    int fail = 0;
    if (uy == 0) fail = 1;
    else if ((UP ? ux : uy) > fit) fail = 2;
    u128 q = 0;
    if (!fail) {
      if (UP) ux *= p10; else uy *= p10;
      q = ux / uy;
    }
    store_dec128(out, i, signed_i128(q, (x < 0) != (y < 0)));
    return fail;
  }
};

template <typename Op>
static int launch_rows(Op op, int64_t n) {
  hipLaunchKernelGGL(k_rows<Op>, dim3(grid_for(n)), dim3(BG_BLOCK), 0, 0, op,
                     n);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// launch the counting form and read the KINDS counters back
template <int KINDS, typename Op>
static int launch_rows_checked(Op op, const uint8_t* avalid,
                               const uint8_t* bvalid, int64_t n,
                               u64* h_failed) {
  DevBuf<u64> d_failed;
  HIP_TRY(d_failed.alloc(KINDS));
  HIP_TRY(hipMemsetAsync(d_failed, 0, sizeof(u64) * KINDS, 0));
  hipLaunchKernelGGL((k_rows_checked<KINDS, Op>), dim3(grid_for(n)),
                     dim3(BG_BLOCK), 0, 0, op, avalid, bvalid, n,
                     d_failed.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(h_failed, d_failed, sizeof(u64) * KINDS,
                    hipMemcpyDeviceToHost));
  return BG_OK;
}

// the correctly rounded doubles 1e0..1e38
static const double BG_P10_F64[39] = {
    1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,
    1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19,
    1e20, 1e21, 1e22, 1e23, 1e24, 1e25, 1e26, 1e27, 1e28, 1e29,
    1e30, 1e31, 1e32, 1e33, 1e34, 1e35, 1e36, 1e37, 1e38};

static u128 p10_u128(int k) {  // k in [0, 38]
  u128 r = 1;
  while (k-- > 0) r *= 10;
  return r;
}

static bool dec_spec_ok(int32_t precision, int32_t scale) {
  return precision >= 1 && precision <= 38 && scale >= 0 && scale <= precision;
}

extern "C" int bg_cast(const bg_column* src, int32_t to_dtype,
                       int32_t to_precision, int32_t to_scale, int64_t n,
                       void* d_out, int64_t* out_failed) {
  REQUIRE_INIT();
  if (out_failed) *out_failed = 0;
  if (!src || n < 0)
    return set_err(BG_ERR_INVALID, "bg_cast: NULL column or negative n");
  const int32_t from = src->dtype;
  const bool from_int = from == BG_DT_INT32 || from == BG_DT_INT64;
  const bool from_dec = from == BG_DT_DECIMAL128;
  const bool ok_pair =
      (to_dtype == BG_DT_FLOAT64 && (from_int || from_dec)) ||
      (to_dtype == BG_DT_DECIMAL128 &&
       (from_int || from_dec || from == BG_DT_FLOAT64)) ||
      (to_dtype == BG_DT_INT64 && from == BG_DT_INT32);
  if (!ok_pair) {
    char msg[128];
    snprintf(msg, sizeof(msg), "bg_cast: dtype %d to dtype %d unsupported",
             (int)from, (int)to_dtype);
    return set_err(BG_ERR_UNSUPPORTED, msg);
  }
  if (from_dec && (src->scale < 0 || src->scale > 38))
    return set_err(BG_ERR_INVALID, "bg_cast: source scale outside 0..38");
  if (to_dtype == BG_DT_DECIMAL128 && !dec_spec_ok(to_precision, to_scale))
    return set_err(BG_ERR_INVALID,
                   "bg_cast: Decimal128 target needs 1 <= precision <= 38 "
                   "and 0 <= scale <= precision");
  if (n == 0) return BG_OK;

  if (to_dtype == BG_DT_FLOAT64) {
    double* out = (double*)d_out;
    if (from == BG_DT_INT32)
      return launch_rows(OpCastToF64<int32_t>{src->d_data, 1.0, out}, n);
    if (from == BG_DT_INT64)
      return launch_rows(OpCastToF64<int64_t>{src->d_data, 1.0, out}, n);
    return launch_rows(
        OpCastToF64<i128>{src->d_data, BG_P10_F64[src->scale], out}, n);
  }
  if (to_dtype == BG_DT_INT64)
    return launch_rows(
        OpCastI32ToI64{(const int32_t*)src->d_data, (int64_t*)d_out}, n);

  // -> Decimal128(to_precision, to_scale).  in_digits bounds the source's
  // decimal digits (0: unknown); a conversion whose widest input still
  // fits the target runs unchecked.
  const uint8_t* valid = src->d_validity;
  u64 failed = 0;
  int rc;
  if (from == BG_DT_FLOAT64) {
    rc = launch_rows_checked<1>(
        OpCastF64ToDec{(const double*)src->d_data, BG_P10_F64[to_scale],
                       p10_u128(to_precision), d_out},
        valid, nullptr, n, &failed);
  } else {
    const int in_digits = from == BG_DT_INT32   ? 10
                          : from == BG_DT_INT64 ? 19
                          : (src->precision >= 1 && src->precision <= 38)
                              ? src->precision : 0;
    const int shift = to_scale - (from_dec ? src->scale : 0);
    if (shift >= 0) {
      const bool fits = in_digits > 0 && in_digits + shift <= to_precision;
      const i128 mul = (i128)p10_u128(shift);
      const u128 bound =
          shift <= to_precision ? p10_u128(to_precision - shift) : (u128)1;
#define BG_CAST_UP(S)                                                       \
  (fits ? launch_rows(OpCastScaleUp<S>{src->d_data, mul, bound, d_out}, n)  \
        : launch_rows_checked<1>(                                           \
              OpCastScaleUp<S>{src->d_data, mul, bound, d_out}, valid,      \
              nullptr, n, &failed))
      rc = from == BG_DT_INT32   ? BG_CAST_UP(int32_t)
           : from == BG_DT_INT64 ? BG_CAST_UP(int64_t)
                                 : BG_CAST_UP(i128);
#undef BG_CAST_UP
    } else {
      // rounding can carry into one more digit: 99.5 -> 100
      const bool fits = in_digits > 0 && in_digits + shift < to_precision;
      const OpCastScaleDown op{src->d_data, p10_u128(-shift),
                               p10_u128(to_precision), d_out};
      rc = fits ? launch_rows(op, n)
                : launch_rows_checked<1>(op, valid, nullptr, n, &failed);
    }
  }
  if (rc != BG_OK) return rc;
  if (out_failed) *out_failed = (int64_t)failed;
  if (failed) {
    char msg[160];
    snprintf(msg, sizeof(msg), "cast: %llu of %lld rows %s Decimal128(%d,%d)",
             failed, (long long)n,
             from == BG_DT_FLOAT64 ? "are NaN, infinite or overflow"
                                   : "overflow",
             (int)to_precision, (int)to_scale);
    return set_err(BG_ERR_INVALID, msg);
  }
  return BG_OK;
}

// Float64 arithmetic, exactly one IEEE-754 binary64 operation per row (no
// fast-math in the build, and no multiply feeds an add here, so
// -ffp-contract has nothing to fuse).  Two rows per lane through 16-byte
// accesses (nvec of them) when every pointer is 16-byte aligned, scalar
// loop for the rest.
template <int OP>
__device__ __forceinline__ double f64_op(double a, double b) {
  switch (OP) {
    case BG_F64_MUL: case BG_F64_MUL_LIT: return a * b;
    case BG_F64_ADD: case BG_F64_ADD_LIT: return a + b;
    case BG_F64_SUB: return a - b;
    case BG_F64_DIV: case BG_F64_DIV_LIT: return a / b;
    case BG_F64_LIT_SUB: return b - a;
    default: return b / a;  // BG_F64_LIT_DIV
  }
}

template <int OP>
__global__ __launch_bounds__(BG_BLOCK) void k_project_f64(
    const double* __restrict__ a, const double* __restrict__ b, double lit,
    int64_t n, int64_t nvec, double* __restrict__ out) {
  typedef double f64x2_pj __attribute__((ext_vector_type(2)));
  constexpr bool BINARY = OP <= BG_F64_DIV;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = tid; v < nvec; v += stride) {
    const f64x2_pj x = reinterpret_cast<const f64x2_pj*>(a)[v];
    f64x2_pj y = {lit, lit};
    if (BINARY) y = reinterpret_cast<const f64x2_pj*>(b)[v];
    f64x2_pj r;
    r[0] = f64_op<OP>(x[0], y[0]);
    r[1] = f64_op<OP>(x[1], y[1]);
    reinterpret_cast<f64x2_pj*>(out)[v] = r;
  }
  for (int64_t i = nvec * 2 + tid; i < n; i += stride)
    out[i] = f64_op<OP>(a[i], BINARY ? b[i] : lit);
}

template <int OP>
static void launch_project_f64(const double* a, const double* b, double lit,
                               int64_t n, double* out) {
  const bool aligned =
      (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15u) == 0;
  const int64_t nvec = aligned ? n / 2 : 0;
  hipLaunchKernelGGL(k_project_f64<OP>, dim3(grid_for(nvec > 0 ? nvec : n)),
                     dim3(BG_BLOCK), 0, 0, a, b, lit, n, nvec, out);
}

extern "C" int bg_project_f64(int32_t op, const bg_column* a,
                              const bg_column* b, double lit, int64_t n,
                              double* d_out) {
  REQUIRE_INIT();
  if (op < BG_F64_MUL || op > BG_F64_LIT_DIV)
    return set_err(BG_ERR_INVALID, "bg_project_f64: unknown op");
  const bool binary = op <= BG_F64_DIV;
  if (!a || (binary && !b))
    return set_err(BG_ERR_INVALID, "bg_project_f64: missing column operand");
  if (a->dtype != BG_DT_FLOAT64 || (binary && b->dtype != BG_DT_FLOAT64))
    return set_err(BG_ERR_INVALID, "bg_project_f64: Float64 columns required");
  if (n < 0) return set_err(BG_ERR_INVALID, "bg_project_f64: negative n");
  if (n == 0) return BG_OK;
  const double* pa = (const double*)a->d_data;
  const double* pb = binary ? (const double*)b->d_data : nullptr;
  switch (op) {
#define BG_F64_CASE(OP) \
  case OP: launch_project_f64<OP>(pa, pb, lit, n, d_out); break
    BG_F64_CASE(BG_F64_MUL);
    BG_F64_CASE(BG_F64_ADD);
    BG_F64_CASE(BG_F64_SUB);
    BG_F64_CASE(BG_F64_DIV);
    BG_F64_CASE(BG_F64_MUL_LIT);
    BG_F64_CASE(BG_F64_ADD_LIT);
    BG_F64_CASE(BG_F64_LIT_SUB);
    BG_F64_CASE(BG_F64_DIV_LIT);
    BG_F64_CASE(BG_F64_LIT_DIV);
#undef BG_F64_CASE
  }
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

extern "C" int bg_div_dec128(const bg_column* a, const bg_column* b,
                             int32_t mul_pow, int64_t n, void* d_out,
                             int64_t* out_failed) {
  REQUIRE_INIT();
  if (out_failed) *out_failed = 0;
  if (!a || !b || n < 0)
    return set_err(BG_ERR_INVALID, "bg_div_dec128: NULL column or negative n");
  if (a->dtype != BG_DT_DECIMAL128 || b->dtype != BG_DT_DECIMAL128)
    return set_err(BG_ERR_INVALID, "bg_div_dec128: Decimal128 columns required");
  if (mul_pow < -38 || mul_pow > 38)
    return set_err(BG_ERR_INVALID, "bg_div_dec128: mul_pow outside -38..38");
  if (n == 0) return BG_OK;
  const u128 p10 = p10_u128(mul_pow < 0 ? -mul_pow : mul_pow);
  const u128 fit = (((u128)1 << 127) - 1) / p10;
  u64 failed[2] = {0, 0};
  const int rc =
      mul_pow >= 0
          ? launch_rows_checked<2>(
                OpDivDec128<true>{a->d_data, b->d_data, p10, fit, d_out},
                a->d_validity, b->d_validity, n, failed)
          : launch_rows_checked<2>(
                OpDivDec128<false>{a->d_data, b->d_data, p10, fit, d_out},
                a->d_validity, b->d_validity, n, failed);
  if (rc != BG_OK) return rc;
  if (out_failed) *out_failed = (int64_t)(failed[0] + failed[1]);
  if (failed[0] || failed[1]) {
    char zero[64] = "", wide[80] = "";
    if (failed[0])
      snprintf(zero, sizeof(zero), "division by zero in %llu row%s", failed[0],
               failed[0] == 1 ? "" : "s");
    if (failed[1])
      snprintf(wide, sizeof(wide), "scaled operand overflows i128 in %llu row%s",
               failed[1], failed[1] == 1 ? "" : "s");
    char msg[192];
    snprintf(msg, sizeof(msg), "div: %s%s%s", zero,
             failed[0] && failed[1] ? ", " : "", wide);
    return set_err(BG_ERR_INVALID, msg);
  }
  return BG_OK;
}

// ---------------------------------------------------------------------------
// Window functions over sorted input (DataFusion's BoundedWindowAggExec /
// WindowAggExec with InputOrderMode::Sorted; Ballista's
// PartitionedBoundedWindowAggExec wraps the former).  The sort is upstream
// (bg_sort_rows2); what runs here is the bandwidth-bound pass over sorted
// rows: partition and peer-group heads as ballot bitmaps, ranks, prefix
// arrays and frame lookups.
//
// Every device-wide scan is hierarchical in SEPARATE launches — per-span
// aggregates, one block scanning the aggregates, a rescan with the carries
// — and no workgroup ever waits for another inside a launch.  A span is
// WIN_SPAN rows (a power of two <= 65536).  One scan kernel serves every
// use: its operator works on (value, has, head) triples, so sums, running
// extrema, restarts at partition heads and NULL inputs are one code path.
// ---------------------------------------------------------------------------
#define WIN_SPAN 4096
#define WIN_OP_SUM 0
#define WIN_OP_MIN 1
#define WIN_OP_MAX 2
#define WIN_HAS 1u   // the element carries a value (a non-NULL input so far)
#define WIN_HEAD 2u  // the element starts a segment (or contains a start)

template <class T>
struct WinElem {
  T v;
  uint32_t fl;
};

// wrap-exact adds: Int64 and Decimal128 sums are arithmetic mod 2^64/2^128
__device__ __forceinline__ i64 win_add(i64 a, i64 b) {
  return (i64)((u64)a + (u64)b);
}
__device__ __forceinline__ i128 win_add(i128 a, i128 b) {
  return (i128)((u128)a + (u128)b);
}
__device__ __forceinline__ double win_add(double a, double b) { return a + b; }
__device__ __forceinline__ i64 win_sub(i64 a, i64 b) {
  return (i64)((u64)a - (u64)b);
}
__device__ __forceinline__ i128 win_sub(i128 a, i128 b) {
  return (i128)((u128)a - (u128)b);
}
__device__ __forceinline__ double win_sub(double a, double b) { return a - b; }

template <class T>
__device__ __forceinline__ T win_op(int op, T a, T b) {
  if (op == WIN_OP_SUM) return win_add(a, b);
  if (op == WIN_OP_MIN) return b < a ? b : a;
  return b > a ? b : a;
}

// the segmented-scan operator: a head on the right discards the left
template <class T>
__device__ __forceinline__ WinElem<T> win_combine(int op, const WinElem<T>& a,
                                                  const WinElem<T>& b) {
  if (b.fl & WIN_HEAD) return b;
  WinElem<T> r;
  r.fl = a.fl | b.fl;
  r.v = (a.fl & b.fl & WIN_HAS) ? win_op(op, a.v, b.v)
                                : ((b.fl & WIN_HAS) ? b.v : a.v);
  return r;
}

__device__ __forceinline__ i64 win_shfl_up(i64 v, int d) {
  return __shfl_up(v, d, BG_WAVE);
}
__device__ __forceinline__ double win_shfl_up(double v, int d) {
  return __shfl_up(v, d, BG_WAVE);
}
__device__ __forceinline__ i128 win_shfl_up(i128 v, int d) {
  const i64 lo = __shfl_up((i64)(u64)(u128)v, d, BG_WAVE);
  const i64 hi = __shfl_up((i64)(u64)((u128)v >> 64), d, BG_WAVE);
  return make_i128((u64)lo, hi);
}

// IEEE total order as a signed i64 (its own inverse): the order of
// k_key_transform_f64 and BG_AGG_OP_MIN_F64
__device__ __forceinline__ i64 win_f64_key(i64 bits) {
  return bits ^ ((bits >> 63) & 0x7FFFFFFFFFFFFFFFll);
}

// a value column as a scan reads it
struct WinSrc {
  const void* data;
  const uint8_t* valid;
  int dtype;  // BG_DT_*; FLOAT64 read as i64 is its total-order key
};

template <class T>
__device__ __forceinline__ T win_load(const WinSrc& s, int64_t i);
template <>
__device__ __forceinline__ i64 win_load<i64>(const WinSrc& s, int64_t i) {
  switch (s.dtype) {
    case BG_DT_INT32:
    case BG_DT_DATE32:
      return (i64) reinterpret_cast<const int32_t*>(s.data)[i];
    case BG_DT_FLOAT64:
      return win_f64_key(reinterpret_cast<const i64*>(s.data)[i]);
    default:
      return reinterpret_cast<const i64*>(s.data)[i];
  }
}
template <>
__device__ __forceinline__ double win_load<double>(const WinSrc& s,
                                                   int64_t i) {
  return reinterpret_cast<const double*>(s.data)[i];
}
template <>
__device__ __forceinline__ i128 win_load<i128>(const WinSrc& s, int64_t i) {
  return load_dec128(s.data, i);
}

template <class T>
struct WinScanArgs {
  WinSrc src;                  // column mode (elems == NULL)
  WinElem<T>* elems;           // element mode: scanned in place
  const uint32_t* part_start;  // row i heads a segment iff part_start[i] == i
  int op;
  int64_t n;
  WinElem<T>* blk;          // aggregate phase: one total per span, no writes
  const WinElem<T>* carry;  // write phase: inclusive-scanned span totals
  T* out;                   // write phase, column mode: inclusive prefix
  u64* has_words;           // optional ballot of WIN_HAS per row
};

// One block walks a span in 256-row tiles: wave scan by shuffles, the four
// wave totals through LDS (two buffers, so one barrier per tile), a running
// carry in registers.
template <class T>
__global__ void __launch_bounds__(BG_BLOCK)
    k_win_scan(WinScanArgs<T> a, int64_t nspans, int64_t span) {
  constexpr int NW = BG_BLOCK / BG_WAVE;
  __shared__ WinElem<T> wtot[2][NW];
  const int lane = lane_id(), wv = threadIdx.x / BG_WAVE;
  int par = 0;  // never reset: consecutive tiles alternate across spans too
  for (int64_t sp = blockIdx.x; sp < nspans; sp += gridDim.x) {
    WinElem<T> run;
    run.v = (T)0;
    run.fl = 0;
    if (a.carry && sp > 0) run = a.carry[sp - 1];
    const int64_t s0 = sp * span;
    const int64_t s1 = s0 + span < a.n ? s0 + span : a.n;
    for (int64_t base = s0; base < s1; base += BG_BLOCK, par ^= 1) {
      const int64_t i = base + threadIdx.x;
      WinElem<T> x;
      x.v = (T)0;
      x.fl = 0;
      if (i < s1) {
        if (a.elems) {
          x = a.elems[i];
        } else {
          if (bit_valid(a.src.valid, i)) {
            x.v = win_load<T>(a.src, i);
            x.fl = WIN_HAS;
          }
          if (a.part_start && a.part_start[i] == (uint32_t)i)
            x.fl |= WIN_HEAD;
        }
      }
#pragma unroll
      for (int d = 1; d < BG_WAVE; d <<= 1) {
        WinElem<T> o;
        o.v = win_shfl_up(x.v, d);
        o.fl = __shfl_up(x.fl, d, BG_WAVE);
        if (lane >= d) x = win_combine(a.op, o, x);
      }
      if (lane == BG_WAVE - 1) wtot[par][wv] = x;
      __syncthreads();
      WinElem<T> acc = run, mine = run;
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        if (k == wv) mine = acc;
        acc = win_combine(a.op, acc, wtot[par][k]);
      }
      x = win_combine(a.op, mine, x);
      run = acc;
      if (a.blk == nullptr) {
        if (i < s1) {
          if (a.elems) a.elems[i] = x;
          else a.out[i] = x.v;
        }
        if (a.has_words) {
          const u64 m = __ballot(i < s1 && (x.fl & WIN_HAS));
          const int64_t w0 = base + (int64_t)wv * BG_WAVE;
          if (lane == 0 && w0 < s1) a.has_words[w0 >> 6] = m;
        }
      }
    }
    if (a.blk && threadIdx.x == 0) a.blk[sp] = run;
  }
}

// Inclusive (optionally segmented) scan of a column: out[i] = the running
// op over the rows of i's segment up to i, NULL inputs skipped.
template <class T>
static int win_scan(const WinSrc& src, const uint32_t* d_part_start, int op,
                    int64_t n, T* d_out, u64* d_has_words) {
  const int64_t nsp = (n + WIN_SPAN - 1) / WIN_SPAN;
  DevBuf<WinElem<T>> d_blk;
  WinScanArgs<T> a{};
  a.src = src;
  a.part_start = d_part_start;
  a.op = op;
  a.n = n;
  const int blocks = (int)bg_imin64(nsp, BG_MAX_BLOCKS);
  if (nsp > 1) {
    HIP_TRY(d_blk.alloc(nsp));
    a.blk = d_blk;
    hipLaunchKernelGGL(k_win_scan<T>, dim3(blocks), dim3(BG_BLOCK), 0, 0, a,
                       nsp, (int64_t)WIN_SPAN);
    WinScanArgs<T> c{};
    c.elems = d_blk;
    c.op = op;
    c.n = nsp;
    hipLaunchKernelGGL(k_win_scan<T>, dim3(1), dim3(BG_BLOCK), 0, 0, c,
                       (int64_t)1, nsp);
    a.carry = d_blk;
  }
  a.blk = nullptr;
  a.out = d_out;
  a.has_words = d_has_words;
  hipLaunchKernelGGL(k_win_scan<T>, dim3(blocks), dim3(BG_BLOCK), 0, 0, a, nsp,
                     (int64_t)WIN_SPAN);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---- head bitmaps and the [start, end) arrays they imply ----

// One thread per row compares row i with row i-1; a wave's 64 verdicts
// leave as one ballot word, so both head sets are Arrow bitmaps.
__global__ void k_win_heads(KeyArgs part, KeyArgs order, int64_t n,
                            u64* part_words, u64* peer_words,
                            int64_t nwords) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t w = wave_global; w < nwords; w += nwaves) {
    const int64_t row = w * BG_WAVE + lane_id();
    bool ph = false, qh = false;
    if (row < n) {
      ph = row == 0 || !keys_equal_rows(part, row - 1, row);
      qh = ph || !keys_equal_rows(order, row - 1, row);
    }
    const u64 pm = __ballot(ph), qm = __ballot(qh);
    if (lane_id() == 0) {
      part_words[w] = pm;
      peer_words[w] = qm;
    }
  }
}

// Per word: its last set bit's row (-1: none) for the forward max scan, and
// minus its first set bit's row (-n: none), stored in reverse word order,
// so the backward min scan is a forward max scan too.
__global__ void k_win_word_edges(const u64* words, int64_t nwords, int64_t n,
                                 i64* fwd, i64* bwd) {
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords;
       w += (int64_t)gridDim.x * blockDim.x) {
    const u64 m = words[w];
    fwd[w] = m ? w * 64 + 63 - __clzll((long long)m) : -1;
    bwd[nwords - 1 - w] = m ? -(w * 64 + (__ffsll((long long)m) - 1)) : -n;
  }
}

// start[i] = the previous set bit at or before i, end[i] = the next set bit
// after i (or n): inside the word by clz/ctz on the masked word, across
// words from the two scanned carry arrays.  Every result is clamped, so no
// input can produce an index outside [0, n].
__global__ void k_win_bounds_fill(const u64* words, const i64* fwd_scan,
                                  const i64* bwd_scan, int64_t nwords,
                                  int64_t n, uint32_t* start_out,
                                  uint32_t* end_out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t w = i >> 6;
    const int l = (int)(i & 63);
    const u64 m = words[w];
    if (start_out) {
      const u64 le = m & (~0ull >> (63 - l));
      int64_t s = le ? w * 64 + 63 - __clzll((long long)le)
                     : (w > 0 ? fwd_scan[w - 1] : 0);
      if (s < 0) s = 0;
      if (s > i) s = i;
      start_out[i] = (uint32_t)s;
    }
    if (end_out) {
      const u64 gt = l == 63 ? 0ull : m & (~0ull << (l + 1));
      int64_t e = gt ? w * 64 + (__ffsll((long long)gt) - 1)
                     : (w + 1 < nwords ? -bwd_scan[nwords - 2 - w] : n);
      if (e <= i) e = i + 1;
      if (e > n) e = n;
      end_out[i] = (uint32_t)e;
    }
  }
}

static void win_key_args(const bg_column* cols, int32_t ncols, KeyArgs* a) {
  a->nkeys = ncols;
  for (int i = 0; i < ncols; ++i) {
    a->k[i].data = cols[i].d_data;
    a->k[i].valid = cols[i].d_validity;
    a->k[i].offsets = cols[i].d_offsets;
    // Float64 keys compare by bit pattern: -0.0 and +0.0 differ, equal NaN
    // patterns match (k_key_transform_f64's total order)
    a->k[i].dtype =
        cols[i].dtype == BG_DT_FLOAT64 ? (int)BG_DT_INT64 : cols[i].dtype;
  }
}

static int win_check_n(const char* who, int64_t n) {
  if (n < 0 || n > (int64_t)UINT32_MAX - 1) {
    char msg[96];
    snprintf(msg, sizeof(msg), "%s: n outside [0, 2^32 - 2]", who);
    return set_err(BG_ERR_INVALID, msg);
  }
  return BG_OK;
}

// start/end arrays of one head bitmap; either output may be NULL
static int win_bounds_of(const u64* d_words, int64_t nwords, int64_t n,
                         i64* d_fwd, i64* d_bwd, i64* d_fscan, i64* d_bscan,
                         uint32_t* d_start, uint32_t* d_end) {
  if (!d_start && !d_end) return BG_OK;
  hipLaunchKernelGGL(k_win_word_edges, dim3(grid_for(nwords)), dim3(BG_BLOCK),
                     0, 0, d_words, nwords, n, d_fwd, d_bwd);
  const WinSrc f{d_fwd, nullptr, BG_DT_INT64}, b{d_bwd, nullptr, BG_DT_INT64};
  int rc = win_scan<i64>(f, nullptr, WIN_OP_MAX, nwords, d_fscan, nullptr);
  if (rc != BG_OK) return rc;
  rc = win_scan<i64>(b, nullptr, WIN_OP_MAX, nwords, d_bscan, nullptr);
  if (rc != BG_OK) return rc;
  hipLaunchKernelGGL(k_win_bounds_fill, dim3(grid_for(n)), dim3(BG_BLOCK), 0,
                     0, d_words, d_fscan, d_bscan, nwords, n, d_start, d_end);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

extern "C" int bg_window_bounds(const bg_column* part_cols, int32_t npart,
                                const bg_column* order_cols, int32_t norder,
                                int64_t n, uint32_t* d_part_start,
                                uint32_t* d_part_end, uint32_t* d_peer_start,
                                uint32_t* d_peer_end) {
  REQUIRE_INIT();
  if (npart < 0 || npart > BG_MAX_KEYS || norder < 0 || norder > BG_MAX_KEYS)
    return set_err(BG_ERR_INVALID,
                   "bg_window_bounds: 0-4 partition and 0-4 order columns");
  if ((npart > 0 && !part_cols) || (norder > 0 && !order_cols))
    return set_err(BG_ERR_INVALID, "bg_window_bounds: NULL key columns");
  if (int rc = win_check_n("bg_window_bounds", n)) return rc;
  if (n == 0) return BG_OK;
  KeyArgs pk{}, ok{};
  win_key_args(part_cols, npart, &pk);
  win_key_args(order_cols, norder, &ok);
  const int64_t nwords = (n + 63) / 64;
  DevBuf<u64> d_part_words, d_peer_words;
  DevBuf<i64> d_fwd, d_bwd, d_fscan, d_bscan;
  HIP_TRY(d_part_words.alloc(nwords));
  HIP_TRY(d_peer_words.alloc(nwords));
  HIP_TRY(d_fwd.alloc(nwords));
  HIP_TRY(d_bwd.alloc(nwords));
  HIP_TRY(d_fscan.alloc(nwords));
  HIP_TRY(d_bscan.alloc(nwords));
  hipLaunchKernelGGL(k_win_heads, dim3(grid_for(n)), dim3(BG_BLOCK), 0, 0, pk,
                     ok, n, d_part_words.get(), d_peer_words.get(), nwords);
  HIP_TRY(hipGetLastError());
  int rc = win_bounds_of(d_part_words, nwords, n, d_fwd, d_bwd, d_fscan,
                         d_bscan, d_part_start, d_part_end);
  if (rc != BG_OK) return rc;
  return win_bounds_of(d_peer_words, nwords, n, d_fwd, d_bwd, d_fscan, d_bscan,
                       d_peer_start, d_peer_end);
}

// ---- counting prefixes over a bitmap ----

// A row set as ballot words plus their popcounts: a validity bitmap read
// bit by bit (so no byte past ceil(n/8) is touched), or the rows that head
// their own group (self[i] == i).
__global__ void k_win_flag_words(const uint8_t* valid, const uint32_t* self,
                                 int64_t n, u64* words, uint32_t* pops,
                                 int64_t nwords) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  for (int64_t w = wave_global; w < nwords; w += nwaves) {
    const int64_t row = w * BG_WAVE + lane_id();
    bool f = false;
    if (row < n) f = valid ? bit_valid(valid, row) : self[row] == (uint32_t)row;
    const u64 m = __ballot(f);
    if (lane_id() == 0) {
      words[w] = m;
      pops[w] = (uint32_t)__popcll(m);
    }
  }
}

// words == NULL: every row is in the set
struct WinCnt {
  const u64* words;
  const i64* pre;  // exclusive prefix of the words' popcounts
};

// members of the set among rows [0, j]
__device__ __forceinline__ int64_t win_cnt_incl(const WinCnt& c, int64_t j) {
  if (!c.words) return j + 1;
  return c.pre[j >> 6] +
         __popcll(c.words[j >> 6] & (~0ull >> (63 - (int)(j & 63))));
}

struct WinCntBufs {
  DevBuf<u64> words;
  DevBuf<uint32_t> pops;
  DevBuf<i64> pre;
};

static int win_count_prefix(const uint8_t* d_valid, const uint32_t* d_self,
                            int64_t n, WinCntBufs* b, WinCnt* out) {
  const int64_t nwords = (n + 63) / 64;
  HIP_TRY(b->words.alloc(nwords));
  HIP_TRY(b->pops.alloc(nwords));
  HIP_TRY(b->pre.alloc(nwords));
  hipLaunchKernelGGL(k_win_flag_words, dim3(grid_for(n)), dim3(BG_BLOCK), 0, 0,
                     d_valid, d_self, n, b->words.get(), b->pops.get(), nwords);
  HIP_TRY(hipGetLastError());
  if (int rc = scan_exclusive_u32(b->pops, nwords, b->pre, nullptr)) return rc;
  out->words = b->words;
  out->pre = b->pre;
  return BG_OK;
}

// ---- ranking ----

__global__ void k_win_rank(int32_t fn, const uint32_t* part_start,
                           const uint32_t* peer_start, WinCnt heads, int64_t n,
                           int64_t* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t ps = part_start ? (int64_t)part_start[i] : 0;
    if (ps > i) ps = i;
    int64_t r;
    if (fn == BG_WIN_ROW_NUMBER) {
      r = i - ps + 1;
    } else if (fn == BG_WIN_RANK) {
      int64_t q = peer_start[i];
      if (q > i) q = i;
      if (q < ps) q = ps;
      r = q - ps + 1;
    } else {  // peer-group heads in (ps, i], plus the partition's own
      r = win_cnt_incl(heads, i) - win_cnt_incl(heads, ps) + 1;
    }
    out[i] = r;
  }
}

extern "C" int bg_window_rank(int32_t fn, const uint32_t* d_part_start,
                              const uint32_t* d_peer_start, int64_t n,
                              int64_t* d_out) {
  REQUIRE_INIT();
  if (fn != BG_WIN_ROW_NUMBER && fn != BG_WIN_RANK && fn != BG_WIN_DENSE_RANK)
    return set_err(BG_ERR_INVALID, "bg_window_rank: unknown fn");
  if (int rc = win_check_n("bg_window_rank", n)) return rc;
  if (n == 0) return BG_OK;
  if (!d_out || (fn != BG_WIN_ROW_NUMBER && !d_peer_start))
    return set_err(BG_ERR_INVALID,
                   "bg_window_rank: NULL output or peer starts");
  WinCntBufs bufs;
  WinCnt heads{nullptr, nullptr};
  if (fn == BG_WIN_DENSE_RANK)
    if (int rc = win_count_prefix(nullptr, d_peer_start, n, &bufs, &heads))
      return rc;
  hipLaunchKernelGGL(k_win_rank, dim3(grid_for(n)), dim3(BG_BLOCK), 0, 0, fn,
                     d_part_start, d_peer_start, heads, n, d_out);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---- frames ----

struct WinFrameArgs {
  int units, start_kind, end_kind, descending;
  int64_t start_off, end_off;  // i64, or f64 bits for a FLOAT64 range key
  WinSrc key;                  // data == NULL: no RANGE offset bound
  const uint32_t *part_start, *part_end, *peer_start, *peer_end;
  int64_t n;
  uint32_t *lo, *hi;
};

// First row of [a, b) whose key is at or after t in the sort direction
// (strict: after t).  The step count is bounded: b - a < 2^32.
template <class K>
__device__ __forceinline__ int64_t win_search(const WinSrc& key, int64_t a,
                                              int64_t b, K t, bool desc,
                                              bool strict) {
  int64_t l = a, r = b;
  for (int it = 0; it < 33 && l < r; ++it) {
    const int64_t m = l + ((r - l) >> 1);
    const K k = win_load<K>(key, m);
    const bool p = strict ? (desc ? k < t : k > t) : (desc ? k <= t : k >= t);
    if (p) r = m;
    else l = m + 1;
  }
  return l;
}

__device__ __forceinline__ i64 win_sat_add(i64 a, i64 b) {
  i64 r;
  if (__builtin_add_overflow(a, b, &r))
    return b < 0 ? (i64)0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFll;
  return r;
}

// the row a RANGE offset bound resolves to; delta is the signed offset
// along the sort direction (preceding < 0 < following)
__device__ __forceinline__ int64_t win_range_bound(const WinFrameArgs& f,
                                                   int64_t i, int64_t a,
                                                   int64_t b, bool following,
                                                   int64_t off, bool is_end) {
  if (f.key.dtype == BG_DT_FLOAT64) {
    double x;
    __builtin_memcpy(&x, &off, 8);
    const double d = following ? x : -x;
    const double k = win_load<double>(f.key, i);
    return win_search<double>(f.key, a, b, f.descending ? k - d : k + d,
                              f.descending != 0, is_end);
  }
  const i64 d = following ? off : -off;
  const i64 k = win_load<i64>(f.key, i);
  return win_search<i64>(f.key, a, b,
                         f.descending ? win_sat_add(k, -d) : win_sat_add(k, d),
                         f.descending != 0, is_end);
}

__global__ void k_win_frame(WinFrameArgs f) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < f.n;
       i += (int64_t)gridDim.x * blockDim.x) {
    // partition and peer group of row i, forced to ps <= qs <= i < qe <= pe
    int64_t ps = f.part_start[i], pe = f.part_end[i];
    if (ps > i) ps = i;
    if (pe <= i) pe = i + 1;
    if (pe > f.n) pe = f.n;
    int64_t lo, hi;
    if (f.units == BG_WIN_ROWS) {
      const int64_t so = f.start_off < f.n ? f.start_off : f.n;
      const int64_t eo = f.end_off < f.n ? f.end_off : f.n;
      lo = f.start_kind == BG_WIN_UNBOUNDED     ? ps
           : f.start_kind == BG_WIN_CURRENT_ROW ? i
           : f.start_kind == BG_WIN_PRECEDING   ? i - so
                                                : i + so;
      hi = f.end_kind == BG_WIN_UNBOUNDED     ? pe
           : f.end_kind == BG_WIN_CURRENT_ROW ? i + 1
           : f.end_kind == BG_WIN_FOLLOWING   ? i + eo + 1
                                              : i - eo + 1;
    } else {
      int64_t qs = f.peer_start[i], qe = f.peer_end[i];
      if (qs > i) qs = i;
      if (qs < ps) qs = ps;
      if (qe <= i) qe = i + 1;
      if (qe > pe) qe = pe;
      const bool s_off = f.start_kind >= BG_WIN_PRECEDING;
      const bool e_off = f.end_kind >= BG_WIN_PRECEDING;
      lo = f.start_kind == BG_WIN_UNBOUNDED ? ps : qs;
      hi = f.end_kind == BG_WIN_UNBOUNDED ? pe : qe;
      // a NULL key keeps its NULL peer group as the offset side
      if ((s_off || e_off) && bit_valid(f.key.valid, i)) {
        // the partition's non-NULL rows [a, b): its NULLs are one peer
        // group at one end
        int64_t a = ps, b = pe;
        if (f.key.valid) {
          if (!bit_valid(f.key.valid, ps)) {
            a = f.peer_end[ps];
            if (a <= ps) a = ps + 1;
            if (a > pe) a = pe;
          } else if (!bit_valid(f.key.valid, pe - 1)) {
            b = f.peer_start[pe - 1];
            if (b > pe - 1) b = pe - 1;
            if (b < ps) b = ps;
          }
        }
        if (s_off)
          lo = win_range_bound(f, i, a, b, f.start_kind == BG_WIN_FOLLOWING,
                               f.start_off, false);
        if (e_off)
          hi = win_range_bound(f, i, a, b, f.end_kind == BG_WIN_FOLLOWING,
                               f.end_off, true);
      }
    }
    if (lo < ps) lo = ps;
    if (lo > pe) lo = pe;
    if (hi > pe) hi = pe;
    if (hi < lo) hi = lo;
    f.lo[i] = (uint32_t)lo;
    f.hi[i] = (uint32_t)hi;
  }
}

extern "C" int bg_window_frame(int32_t units, int32_t start_kind,
                               int64_t start_off, int32_t end_kind,
                               int64_t end_off, const bg_column* order_col,
                               int32_t descending,
                               const uint32_t* d_part_start,
                               const uint32_t* d_part_end,
                               const uint32_t* d_peer_start,
                               const uint32_t* d_peer_end, int64_t n,
                               uint32_t* d_lo, uint32_t* d_hi) {
  REQUIRE_INIT();
  if (units != BG_WIN_ROWS && units != BG_WIN_RANGE)
    return set_err(BG_ERR_UNSUPPORTED,
                   "bg_window_frame: units must be ROWS or RANGE");
  auto kind_ok = [](int32_t k) {
    return k >= BG_WIN_UNBOUNDED && k <= BG_WIN_FOLLOWING;
  };
  if (!kind_ok(start_kind) || !kind_ok(end_kind))
    return set_err(BG_ERR_INVALID, "bg_window_frame: unknown bound kind");
  const bool s_off = start_kind >= BG_WIN_PRECEDING;
  const bool e_off = end_kind >= BG_WIN_PRECEDING;
  const bool range_off = units == BG_WIN_RANGE && (s_off || e_off);
  const bool f64 = range_off && order_col && order_col->dtype == BG_DT_FLOAT64;
  auto off_ok = [f64](int64_t off) {
    if (!f64) return off >= 0;
    double x;
    memcpy(&x, &off, 8);
    return x >= 0.0;  // false for NaN as well
  };
  if ((s_off && !off_ok(start_off)) || (e_off && !off_ok(end_off)))
    return set_err(BG_ERR_INVALID, "bg_window_frame: negative offset");
  if (range_off) {
    if (!order_col)
      return set_err(BG_ERR_INVALID,
                     "bg_window_frame: a RANGE offset needs the order column");
    const int32_t dt = order_col->dtype;
    if (dt != BG_DT_INT64 && dt != BG_DT_INT32 && dt != BG_DT_DATE32 &&
        dt != BG_DT_FLOAT64)
      return set_err(BG_ERR_UNSUPPORTED,
                     "bg_window_frame: RANGE offset over a key that is not "
                     "Int64/Int32/Date32/Float64");
  }
  if (int rc = win_check_n("bg_window_frame", n)) return rc;
  if (n == 0) return BG_OK;
  if (!d_part_start || !d_part_end || !d_lo || !d_hi ||
      (units == BG_WIN_RANGE && (!d_peer_start || !d_peer_end)))
    return set_err(BG_ERR_INVALID, "bg_window_frame: NULL bounds array");
  WinFrameArgs f{};
  f.units = units;
  f.start_kind = start_kind;
  f.end_kind = end_kind;
  f.descending = descending ? 1 : 0;
  f.start_off = s_off ? start_off : 0;
  f.end_off = e_off ? end_off : 0;
  if (range_off)
    f.key = WinSrc{order_col->d_data, order_col->d_validity, order_col->dtype};
  f.part_start = d_part_start;
  f.part_end = d_part_end;
  f.peer_start = d_peer_start;
  f.peer_end = d_peer_end;
  f.n = n;
  f.lo = d_lo;
  f.hi = d_hi;
  hipLaunchKernelGGL(k_win_frame, dim3(grid_for(n)), dim3(BG_BLOCK), 0, 0, f);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

// ---- aggregates over a frame ----

template <class T>
struct WinFinishArgs {
  int fn;             // BG_WIN_SUM / COUNT / MIN / MAX
  int out_dtype;      // how a value leaves: BG_DT_*
  int seg;            // the prefix restarts at every partition start
  const T* prefix;    // inclusive prefix / running extremum (NULL: count)
  const u64* has_words;  // MIN/MAX: rows whose running extremum exists
  WinCnt cnt;            // non-NULL inputs
  const uint32_t *part_start, *lo, *hi;
  int64_t n;
  void* out;
  uint8_t* valid_out;
};

__device__ __forceinline__ void win_store(void* out, int dt, int64_t i,
                                          i64 v) {
  if (dt == BG_DT_INT32 || dt == BG_DT_DATE32)
    reinterpret_cast<int32_t*>(out)[i] = (int32_t)v;
  else if (dt == BG_DT_FLOAT64)  // a total-order key back to its bits
    reinterpret_cast<i64*>(out)[i] = win_f64_key(v);
  else
    reinterpret_cast<i64*>(out)[i] = v;
}
__device__ __forceinline__ void win_store(void* out, int, int64_t i,
                                          double v) {
  reinterpret_cast<double*>(out)[i] = v;
}
__device__ __forceinline__ void win_store(void* out, int, int64_t i, i128 v) {
  ulong2 o;
  o.x = (u64)(u128)v;
  o.y = (u64)((u128)v >> 64);
  reinterpret_cast<ulong2*>(out)[i] = o;
}

// One thread per row reads the prefix at its frame's two ends.  Whole waves
// iterate, so a wave's 64 validity verdicts are one ballot and eight lanes
// store its bytes: ceil(n/8) bytes written whole, none beyond.
template <class T>
__global__ void k_win_agg_finish(WinFinishArgs<T> a, int64_t nwords) {
  const int64_t wave_global =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / BG_WAVE;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) / BG_WAVE;
  const int64_t nbytes = (a.n + 7) / 8;
  for (int64_t w = wave_global; w < nwords; w += nwaves) {
    const int64_t i = w * BG_WAVE + lane_id();
    bool ok = false;
    if (i < a.n) {
      int64_t ps = a.part_start ? (int64_t)a.part_start[i] : 0;
      if (ps > i) ps = i;
      int64_t lo = a.lo ? (int64_t)a.lo[i] : ps;
      int64_t hi = a.hi[i];
      if (lo > a.n) lo = a.n;
      if (hi > a.n) hi = a.n;
      if (hi < lo) hi = lo;
      if (a.fn == BG_WIN_COUNT || a.fn == BG_WIN_SUM) {
        int64_t c = 0;
        if (hi > lo)
          c = win_cnt_incl(a.cnt, hi - 1) -
              (lo > 0 ? win_cnt_incl(a.cnt, lo - 1) : 0);
        ok = c > 0;
        if (a.fn == BG_WIN_COUNT) {
          reinterpret_cast<i64*>(a.out)[i] = c;
        } else {
          T s = (T)0;
          if (ok) {
            s = a.prefix[hi - 1];
            if (lo > (a.seg ? ps : 0)) s = win_sub(s, a.prefix[lo - 1]);
          }
          win_store(a.out, a.out_dtype, i, s);
        }
      } else {
        ok = hi > lo && ((a.has_words[(hi - 1) >> 6] >> ((hi - 1) & 63)) & 1);
        win_store(a.out, a.out_dtype, i, ok ? a.prefix[hi - 1] : (T)0);
      }
    }
    const u64 m = __ballot(ok);
    if (a.valid_out && lane_id() < 8 && w * 8 + lane_id() < nbytes)
      a.valid_out[w * 8 + lane_id()] = (uint8_t)(m >> (8 * lane_id()));
  }
}

// prefix (and, for MIN/MAX, the has bitmap) of val, then the per-row pass
template <class T>
static int win_agg_run(int32_t fn, const bg_column* val, int seg,
                       const WinCnt& cnt, const uint32_t* d_part_start,
                       const uint32_t* d_lo, const uint32_t* d_hi, int64_t n,
                       void* d_out, uint8_t* d_valid_out) {
  const int64_t nwords = (n + 63) / 64;
  const bool extremum = fn == BG_WIN_MIN || fn == BG_WIN_MAX;
  DevBuf<T> d_prefix;
  DevBuf<u64> d_has;
  WinFinishArgs<T> a{};
  a.fn = fn;
  a.seg = seg;
  a.cnt = cnt;
  a.part_start = d_part_start;
  a.lo = d_lo;
  a.hi = d_hi;
  a.n = n;
  a.out = d_out;
  a.valid_out = d_valid_out;
  if (fn != BG_WIN_COUNT) {
    HIP_TRY(d_prefix.alloc(n));
    if (extremum) HIP_TRY(d_has.alloc(nwords));
    const WinSrc src{val->d_data, val->d_validity, val->dtype};
    const int op = fn == BG_WIN_SUM   ? WIN_OP_SUM
                   : fn == BG_WIN_MIN ? WIN_OP_MIN
                                      : WIN_OP_MAX;
    if (int rc = win_scan<T>(src, seg ? d_part_start : nullptr, op, n,
                             d_prefix.get(), extremum ? d_has.get() : nullptr))
      return rc;
    a.prefix = d_prefix;
    a.has_words = d_has;
    a.out_dtype = val->dtype;
  }
  hipLaunchKernelGGL(k_win_agg_finish<T>, dim3(grid_for(n)), dim3(BG_BLOCK), 0,
                     0, a, nwords);
  HIP_TRY(hipGetLastError());
  return BG_OK;
}

extern "C" int bg_window_agg(int32_t fn, const bg_column* val,
                             const uint32_t* d_part_start,
                             const uint32_t* d_lo, const uint32_t* d_hi,
                             int64_t n, void* d_out, uint8_t* d_valid_out) {
  REQUIRE_INIT();
  if (fn < BG_WIN_SUM || fn > BG_WIN_MAX)
    return set_err(BG_ERR_INVALID, "bg_window_agg: unknown fn");
  const bool extremum = fn == BG_WIN_MIN || fn == BG_WIN_MAX;
  if (extremum && d_lo)
    return set_err(BG_ERR_UNSUPPORTED,
                   "bg_window_agg: MIN/MAX only over frames that start at the "
                   "partition start (d_lo must be NULL); a sliding extremum "
                   "is not implemented");
  if (!val && fn != BG_WIN_COUNT)
    return set_err(BG_ERR_INVALID, "bg_window_agg: val is NULL (count only)");
  const int32_t dt = val ? val->dtype : (int32_t)BG_DT_INT64;
  if (fn == BG_WIN_SUM && dt != BG_DT_INT64 && dt != BG_DT_DECIMAL128 &&
      dt != BG_DT_FLOAT64)
    return set_err(BG_ERR_UNSUPPORTED,
                   "bg_window_agg: SUM over Int64/Decimal128/Float64 only");
  if (extremum && dt != BG_DT_INT64 && dt != BG_DT_INT32 &&
      dt != BG_DT_DATE32 && dt != BG_DT_FLOAT64 && dt != BG_DT_DECIMAL128)
    return set_err(BG_ERR_UNSUPPORTED,
                   "bg_window_agg: MIN/MAX over Int64/Int32/Date32/Float64/"
                   "Decimal128 only");
  if (int rc = win_check_n("bg_window_agg", n)) return rc;
  if (n == 0) return BG_OK;
  if (!d_hi || !d_out || (!d_lo && !d_part_start) ||
      (fn != BG_WIN_COUNT && !d_valid_out))
    return set_err(BG_ERR_INVALID, "bg_window_agg: NULL array");
  // non-NULL inputs per frame: a prefix only when the column has a bitmap
  WinCntBufs bufs;
  WinCnt cnt{nullptr, nullptr};
  if (!extremum && val && val->d_validity)
    if (int rc = win_count_prefix(val->d_validity, nullptr, n, &bufs, &cnt))
      return rc;
  if (fn == BG_WIN_COUNT)
    return win_agg_run<i64>(fn, val, 0, cnt, d_part_start, d_lo, d_hi, n, d_out,
                            nullptr);
  if (dt == BG_DT_DECIMAL128)
    return win_agg_run<i128>(fn, val, extremum, cnt, d_part_start, d_lo, d_hi,
                             n, d_out, d_valid_out);
  // a Float64 running sum restarts at every partition start, so one
  // partition's magnitude never cancels into another's
  if (dt == BG_DT_FLOAT64 && fn == BG_WIN_SUM)
    return win_agg_run<double>(fn, val, 1, cnt, d_part_start, d_lo, d_hi, n,
                               d_out, d_valid_out);
  return win_agg_run<i64>(fn, val, extremum, cnt, d_part_start, d_lo, d_hi, n,
                          d_out, d_valid_out);
}
