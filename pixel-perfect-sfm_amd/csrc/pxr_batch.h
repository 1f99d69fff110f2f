// pxr_batch.h -- what the host drivers of the batched stages share (absolute pose, two-view geometry, triangulation, matching):
// the validation of an offsets array with the processing order it gives, the layout of the context's workspace, and the events
// behind the *_timed entry points.
#pragma once
#include <algorithm>
#include <vector>

#include "pxr_internal.h"

namespace pxr {

// how the messages about an offsets array name things: "<fn>: <offsets> is not monotone at <item> 7", "... not at <total> = 9"
struct OffsetNames { const char* fn; const char* offsets; const char* item; const char* total; };

// The T + 1 offsets of a batch of T >= 1 items over N elements, validated on a host copy: off[0] == 0 (or only >= 0 with
// first_may_be_positive), monotone, ending at N; check_item(t) is the driver's own check of item t (PXR_OK or its error), made
// between the monotonicity checks of items t and t + 1.  The copy also gives the processing order: the items by descending
// length (a stable counting sort), so that the longest start first.  The stream is synchronised before the checks: a download
// the driver queued before the call has arrived too.
template <class CheckItem>
inline int batch_order(pxr_ctx* ctx, const OffsetNames& nm, bool first_may_be_positive, const int64_t* d_offsets, int64_t T, int64_t N,
                       std::vector<int64_t>& off, std::vector<int32_t>& order, CheckItem check_item) {
  off.resize((size_t)T + 1);
  PXR_HIP(hipMemcpyAsync(off.data(), d_offsets, sizeof(int64_t) * ((size_t)T + 1), hipMemcpyDeviceToHost, ctx->stream));
  PXR_HIP(hipStreamSynchronize(ctx->stream));
  if (first_may_be_positive) PXR_REQUIRE(off[0] >= 0, "%s: %s[0] = %lld is negative", nm.fn, nm.offsets, (long long)off[0]);
  else PXR_REQUIRE(off[0] == 0, "%s: %s[0] = %lld, not 0", nm.fn, nm.offsets, (long long)off[0]);
  int64_t longest = 0;
  for (int64_t t = 0; t < T; ++t) {
    PXR_REQUIRE(off[t + 1] >= off[t], "%s: %s is not monotone at %s %lld", nm.fn, nm.offsets, nm.item, (long long)t);
    if (int rc = check_item(t)) return rc;
    longest = std::max(longest, off[t + 1] - off[t]);
  }
  PXR_REQUIRE(off[T] == N, "%s: %s ends at %lld, not at %s = %lld", nm.fn, nm.offsets, (long long)off[T], nm.total, (long long)N);
  order.resize((size_t)T);
  std::vector<int64_t> first((size_t)longest + 2, 0);                      // first[longest - len]: where the items of that length begin
  for (int64_t t = 0; t < T; ++t) ++first[(size_t)(longest - (off[t + 1] - off[t])) + 1];
  for (size_t k = 1; k < first.size(); ++k) first[k] += first[k - 1];
  for (int64_t t = 0; t < T; ++t) order[(size_t)first[(size_t)(longest - (off[t + 1] - off[t]))]++] = (int32_t)t;
  return PXR_OK;
}

// The layout of the context's workspace as typed device arrays.  take(p, count) books `count` elements of p's pointee type at
// the next multiple of 256 bytes (a count of 0 takes no room) and remembers where p lives; commit() grows the workspace to the
// total and only then fills every p, so no pointer into the block exists before the block has its final address.  commit()
// leaves the layout empty: a driver that lays out twice in one call takes and commits again, from offset 0, and keeps no pointer
// of the first layout (growing loses the contents).  release_caches: see grow_block.
class Workspace {
 public:
  template <class T>
  void take(T*& p, size_t count) {
    slots_.push_back({&p, bytes_, [](void* at, char* base) { *static_cast<T**>(at) = reinterpret_cast<T*>(base); }});
    bytes_ += (count * sizeof(T) + 255) & ~(size_t)255;
  }
  int commit(pxr_ctx* ctx, bool release_caches = false) {
    if (int rc = grow_workspace(ctx, bytes_, release_caches)) return rc;
    for (const Slot& s : slots_) s.fill(s.at, static_cast<char*>(ctx->d_workspace) + s.offset);
    slots_.clear();
    bytes_ = 0;
    return PXR_OK;
  }

 private:
  struct Slot { void* at; size_t offset; void (*fill)(void* at, char* base); };
  std::vector<Slot> slots_;
  size_t bytes_ = 0;
};

// The events of a *_timed call.  Without h_ms nothing is created and mark() does nothing; the destructor destroys what create()
// made, on every path out of the driver.  MARKS: the marks a driver records (its stages + 1).
template <int MARKS>
class StageTimer {
 public:
  StageTimer(hipStream_t stream, double* h_ms) : st_(stream), h_ms_(h_ms), n_(h_ms ? MARKS : 0) {}
  StageTimer(const StageTimer&) = delete;
  StageTimer& operator=(const StageTimer&) = delete;
  ~StageTimer() { for (int k = 0; k < n_; ++k) if (ev_[k]) (void)hipEventDestroy(ev_[k]); }
  int create(const char* fn) {
    for (int k = 0; k < n_; ++k) if (hipEventCreate(&ev_[k]) != hipSuccess) return set_error(PXR_EHIP, "%s: hipEventCreate failed", fn);
    return PXR_OK;
  }
  void mark(int k) { if (h_ms_) (void)hipEventRecord(ev_[k], st_); }
  // h_ms[k] = milliseconds between marks from[k] and from[k] + 1, k < n (the stream is synchronised first)
  int read(const int* from, int n) {
    if (!h_ms_) return PXR_OK;
    int rc = hip_check(hipStreamSynchronize(st_), "hipStreamSynchronize");
    for (int k = 0; k < n && rc == PXR_OK; ++k) {
      float ms = 0.f;
      rc = hip_check(hipEventElapsedTime(&ms, ev_[from[k]], ev_[from[k] + 1]), "hipEventElapsedTime");
      h_ms_[k] = ms;
    }
    return rc;
  }
  // For a driver whose stages repeat: h_ms[k] += milliseconds between marks k and k + 1 of one round, k < MARKS - 1.  The driver
  // zeroes h_ms when the call starts and adds after the round's own synchronisation (it waits for the round's info word anyway)
  int add() {
    for (int k = 0; k + 1 < n_; ++k) {
      float ms = 0.f;
      if (int rc = hip_check(hipEventElapsedTime(&ms, ev_[k], ev_[k + 1]), "hipEventElapsedTime")) return rc;
      h_ms_[k] += ms;
    }
    return PXR_OK;
  }

 private:
  hipStream_t st_;
  double* h_ms_;
  int n_;
  hipEvent_t ev_[MARKS] = {};
};

}  // namespace pxr
