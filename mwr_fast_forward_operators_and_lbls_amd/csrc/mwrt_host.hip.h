// mwrt_host.hip.h -- what the two host units of libmwrt.so share (csrc/mwrt.hip: context and model lifecycle, the TB,
// absorption, tau and Jacobian entries, the utilities; csrc/mwrt_retrieval.hip: the entries that take a versioned record
// and the handles they use): the context, its device buffers and caches, the one error message of a thread, and the steps
// every *_device entry ends with.  Host code only: no kernel and no kernel unit's header is included here.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mwrt.h"

#include <cstring>
#include <string>
#include <vector>

namespace mwrt {

// the thread's message behind mwrt_last_error (defined in csrc/mwrt.hip); returns `code`
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(e_ == hipErrorOutOfMemory ? MWRT_ERR_OUT_OF_MEMORY : MWRT_ERR_HIP,         \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                        \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <class T> T* as() { return static_cast<T*>(p); }
};

// Content-keyed, immutable device blobs: the small per-call parameter arrays (frq, air mass, elevations), the line
// masks of a frequency list and its window tables.  The key is (model id or 0, a small integer tag, doubles).  A blob is
// never overwritten or freed while the context lives (bar LRU eviction behind a device-wide drain), so launches still
// queued on ANY stream and captured hipGraphs keep reading valid memory.
class DeviceCache {
 public:
  struct Blob { const char* dev = nullptr; int count = 0; };     // count: what the builder returned (records in the blob)
  explicit DeviceCache(size_t capacity) : capacity_(capacity) {}
  // The blob of (model, tag, key[0..n)).  A hit is one linear memcmp scan: it never evicts or synchronises.  On a miss
  // `build(std::vector<char>* host)` fills the host bytes and returns the count; uploads go through `copy_stream`
  // (never a capturing stream).
  template <class Build>
  hipError_t get(uint64_t model, int tag, const double* key, int n, hipStream_t copy_stream, Build build, Blob* out) {
    for (Entry& e : entries_)
      if (e.model == model && e.tag == tag && (int)e.key.size() == n &&
          std::memcmp(e.key.data(), key, sizeof(double) * (size_t)n) == 0) {
        // least recently USED goes first: a hit is stamped anew, so a warm-up call keeps what it touched (a later miss of the
        // same sequence must not evict it -- the eviction drains the device, which a capturing stream refuses)
        e.stamp = ++clock_;
        *out = Blob{e.dev, e.count};
        return hipSuccess;
      }
    std::vector<char> host;
    const int count = build(&host);
    return insert(model, tag, key, n, host, count, copy_stream, out);
  }
  void release() { for (Entry& e : entries_) (void)hipFree(e.dev); entries_.clear(); }
  // the caller has drained the device: launches on any stream may still read the blobs
  void drop_model(uint64_t model) {
    for (size_t i = entries_.size(); i-- > 0;)
      if (entries_[i].model == model) { (void)hipFree(entries_[i].dev); entries_.erase(entries_.begin() + (long)i); }
  }

 private:
  struct Entry { uint64_t model; int tag; std::vector<double> key; char* dev; int count; unsigned long stamp; };
  hipError_t insert(uint64_t model, int tag, const double* key, int n, const std::vector<char>& host, int count,
                    hipStream_t copy_stream, Blob* out) {
    if (entries_.size() >= capacity_) {
      // bounded: evict the least recently used blob -- only after everything queued on the device has drained
      hipError_t e = hipDeviceSynchronize();
      if (e != hipSuccess) return e;
      size_t lru = 0;
      for (size_t i = 1; i < entries_.size(); ++i) if (entries_[i].stamp < entries_[lru].stamp) lru = i;
      (void)hipFree(entries_[lru].dev);
      entries_.erase(entries_.begin() + (long)lru);
    }
    Entry ne{model, tag, std::vector<double>(key, key + n), nullptr, count, 0};
    hipError_t e = hipMalloc((void**)&ne.dev, host.empty() ? 1 : host.size());
    if (e != hipSuccess) return e;
    // a fresh buffer nobody reads yet: copy on the context's own stream and wait for it, so the
    // bytes are in HBM before any stream (the caller's included) can launch a reader
    e = hipMemcpyAsync(ne.dev, host.data(), host.size(), hipMemcpyHostToDevice, copy_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(copy_stream);
    if (e != hipSuccess) { (void)hipFree(ne.dev); return e; }
    ne.stamp = ++clock_;
    entries_.push_back(std::move(ne));
    *out = Blob{entries_.back().dev, count};
    return hipSuccess;
  }
  std::vector<Entry> entries_;
  size_t capacity_;
  unsigned long clock_ = 0;
};

// What a handle that owns one device blob is made of (mwrt_obs, mwrt_basis): created on a context, freed by its own
// *_destroy behind a device-wide drain, or by mwrt_destroy when the context goes first -- the handle then stays valid for
// its *_destroy alone and every entry refuses it (ctx no longer equals the caller's context).
struct DeviceHandle {
  mwrt_context* ctx = nullptr;  // null once the context is gone
  void* d_blob = nullptr;
};

}  // namespace mwrt

struct mwrt_context {
  int device = 0;
  hipStream_t stream = nullptr;
  int lds_max = 65536;
  int num_cus = 256;            // compute units of the device (MI355X: 256)
  // small per-call parameter arrays (frq, airmass, elevations): content-keyed device copies
  mwrt::DeviceCache frq_cache{32}, am_cache{32}, elev_cache{32};
  int absorption_mode = 0;      // 0 auto, 1 direct, 2 windowed
  int chunk_width = 0;          // 0 auto, 8 / 14 / 16: frequencies per workgroup of the fused TB kernel (mwrt_set_chunk_width)
  // fine-grid absorption: window descriptors + Lagrange matrices per (model, frequency list)
  mwrt::DeviceCache win_cache{16};
  // line classification of every frequency chunk (LineMasks), per (model, frequency list, chunk width): depends on the
  // frequencies and the table only, so the host computes it once instead of every workgroup voting on it
  mwrt::DeviceCache mask_cache{64};
  // ray-tracing workspace: path factors [nprof][nang][nlev] and the per-profile ducting flag
  mwrt::DevBuf d_amf, d_duct;
  // fine-grid two-kernel path: materialised absorption of one profile batch (awet | adry)
  mwrt::DevBuf d_alpha;
  size_t alpha_batch_bytes = (size_t)4 << 30;   // 4 GiB of a 288-GB card: configs[4]'s per-GPU share is one batch
  // the two workspaces above are shared by consecutive calls: a call that uses one on a different stream than
  // the previous user first waits (on the device) for that user's last kernel
  hipEvent_t ws_event = nullptr;
  hipStream_t ws_stream = nullptr;
  bool ws_used = false;
  // device K-matrix path: the six tangent-linear absorption arrays + per-profile flags (grown only, never shrunk;
  // handed over between streams like d_amf / d_alpha)
  mwrt::DevBuf d_jac;
  // spectroscopic-parameter Jacobian: d alpha / d b of one group of parameters (grown only, handed over like d_jac) and
  // the content-keyed device copies of the parameter lists
  mwrt::DevBuf d_par;
  mwrt::DeviceCache par_cache{32};
  // staging for the host-buffer entry points
  mwrt::DevBuf d_in, d_out, d_valid, d_ex;
  // timing: a ring of hipEvent pairs recorded around every kernel launch, on the launch stream
  bool timing = false;
  std::vector<hipEvent_t> ev0, ev1;
  long ev_count = 0;
  // instrument operators and reduced bases created on this context and not yet destroyed: mwrt_destroy frees their blobs
  std::vector<mwrt::DeviceHandle*> handles_live;
};

namespace mwrt {

constexpr int TIMING_RING = 512;

// `stream` argument of the *_device entry points: NULL = the context's own (non-blocking) stream,
// MWRT_STREAM_LEGACY = the caller's legacy default stream (hipStream_t 0), else the handle itself
inline hipStream_t resolve_stream(const mwrt_context* c, void* stream) {
  if (!stream) return c->stream;
  if (stream == MWRT_STREAM_LEGACY) return (hipStream_t) nullptr;
  return (hipStream_t)stream;
}

// one kernel launch (`launch()` -> hipError_t), between a pair of the ring's events when timing is on
template <class F> int timed(mwrt_context* c, hipStream_t st, F launch) {
  if (c->timing) (void)hipEventRecord(c->ev0[c->ev_count % TIMING_RING], st);
  const hipError_t e = launch();
  if (c->timing) { (void)hipEventRecord(c->ev1[c->ev_count % TIMING_RING], st); c->ev_count++; }
  HIP_TRY(e);
  return MWRT_OK;
}

}  // namespace mwrt
