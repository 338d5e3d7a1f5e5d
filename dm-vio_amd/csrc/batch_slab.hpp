// The host plumbing every W-windows-per-call entry point shares: where the parts of a call's slab lie (DmvCursor), the slab itself with its device twin and the rule for
// "the pinned side may be rewritten now" (DmvSlab), the refusals of a call's head (dmvBatchHead) and of a handle named twice (dmvFirstRepeated), and what a call enqueued
// and waited for (DmvWork).  The first part makes no HIP call and compiles under a plain host compiler (tests/batch_slab_harness.cpp); it needs failmsg() in scope
// (internal.h; the harness has its own).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

// ---- the ONE alignment rule of the batched calls: every part of a slab starts on a 256-byte boundary
static inline size_t dmvPad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// Offsets only.  take<T>(n): the byte offset of n objects of T; bytes(): what an upload of everything taken so far must cover.
struct DmvCursor {
  size_t off = 0;
  size_t takeBytes(size_t b) { const size_t at = off; off += dmvPad(b); return at; }
  template <class T> size_t take(size_t n) { return takeBytes(sizeof(T) * n); }
  size_t bytes() const { return off; }
};
// The slabs that are sized once, at creation.  A call packs with the functions below and creation reserves what the same functions take at max_windows with every window
// at its largest, so a slab sized at creation holds whatever a call packs (tests/batch_slab_harness.cpp holds them to that).  Every slab starts with its W records, whose
// size is the caller's (kernel headers): dmvRecords().
static inline size_t dmvRecords(DmvCursor& c, size_t rec, int W) { return c.takeBytes(rec * (size_t)W); }
//   trace batch:    [TraceWin x W | per window KRKi 9H, Kt 3H, aff 2H floats]
static inline size_t dmvTraceTable(DmvCursor& c, int n_hosts) { return c.take<float>(14 * (size_t)n_hosts); }
static inline size_t dmvTraceSlabBytes(size_t rec, int max_windows, int max_hosts) {
  DmvCursor c;
  dmvRecords(c, rec, max_windows);
  for (int k = 0; k < max_windows; k++) dmvTraceTable(c, max_hosts);
  return c.bytes();
}
//   selector batch: [SelWin x W | 256 floats per window]
static inline size_t dmvSelLuts(DmvCursor& c, int W) { return c.take<float>(256 * (size_t)W); }
static inline size_t dmvSelSlabBytes(size_t rec, int max_windows) { DmvCursor c; dmvRecords(c, rec, max_windows); dmvSelLuts(c, max_windows); return c.bytes(); }
//   set_ref batch:  [RefWin x W | u, v, idepth, hdiF of every window, floats | a rank byte per point], or from BA windows [RefWin x W | RefBaWin x W]
static inline size_t dmvRefPoints(DmvCursor& c, size_t total) { return c.take<float>(4 * total); }
static inline size_t dmvRefRanks(DmvCursor& c, size_t total) { return c.take<unsigned char>(total); }
static inline size_t dmvRefSlabBytes(size_t rec, size_t ba_rec, int max_windows, int max_points) {
  const size_t total = (size_t)max_windows * (size_t)max_points;
  DmvCursor a, b;
  dmvRecords(a, rec, max_windows); dmvRefPoints(a, total); dmvRefRanks(a, total);
  dmvRecords(b, rec, max_windows); dmvRecords(b, ba_rec, max_windows);
  return std::max(a.bytes(), b.bytes());
}

// ---- the head of a call: no handle, W outside [0, max_windows], no array for W > 0 — in that order.  `text`: the three refusals of a caller that words its own.
static const char* const DMV_HEAD_TEXT[3] = {": null batch handle", ": W is negative or larger than the batch's max_windows", ": the window array is NULL"};
static inline int dmvBatchHead(const void* handle, int W, int max_windows, const void* arr, const char* who, const char* const* text = DMV_HEAD_TEXT) {
  const int k = !handle ? 0 : (W < 0 || W > max_windows) ? 1 : (W > 0 && !arr) ? 2 : -1;
  return k < 0 ? 0 : failmsg(std::string(who) + text[k]);
}
// The first window (lowest index) that names the handle of an earlier window, or -1: what a loop over the windows with an inner loop over the earlier ones finds first,
// in n log n.  The callers word the refusal.
static inline int dmvFirstRepeated(const void* const* handles, int W) {
  std::vector<std::pair<uintptr_t, int>> v((size_t)std::max(W, 0));
  for (int k = 0; k < W; k++) v[k] = {reinterpret_cast<uintptr_t>(handles[k]), k};
  std::sort(v.begin(), v.end());
  int first = -1;   // (inside a run of equal handles the indices ascend: the run's second entry is its first repeat)
  for (size_t i = 1; i < v.size(); i++)
    if (v[i].first == v[i - 1].first && (first < 0 || v[i].second < first)) first = v[i].second;
  return first;
}
template <class WIN, class H>
static inline int dmvFirstRepeated(const WIN* win, int W, H WIN::*handle) {
  std::vector<const void*> p((size_t)std::max(W, 0));
  for (int k = 0; k < W; k++) p[k] = win[k].*handle;
  return dmvFirstRepeated(p.data(), W);
}

// ---- launches, uploads, downloads and waits of a call, counted where they are enqueued (the *_last_work getters)
struct DmvWork {
  int launches = 0, uploads = 0, downloads = 0, waits = 0;
  void clear() { launches = uploads = downloads = waits = 0; }
  void report(int* l, int* u, int* d, int* w) const { if (l) *l = launches; if (u) *u = uploads; if (d) *d = downloads; if (w) *w = waits; }
};

#if defined(__HIPCC__)
// A device buffer with its pinned twin (or two mirrors of it, or none), sized at creation or grown to a call's need.  A call: reserve() where the slab grows, begin(),
// put() for every part, upload(), its kernels, download() where results come back in the slab, wait().  begin() picks the mirror and, where that mirror's last upload is
// not known to have landed, waits for it: for the mirror's event where the slab records one, else for the stream.  wait() (or settled(), behind a wait of the unit's
// own) marks every upload as landed, so a unit that waits at the end of each call never waits in begin().  `work`, where set, counts what upload / download / wait do.
// Not counted: a growth's drain of the stream, and begin()'s wait (reached after a failed call and by the trace batch, which has no work getter).
struct DmvSlab {
  char *d = nullptr, *h[2] = {nullptr, nullptr};
  hipEvent_t landed[2] = {nullptr, nullptr};
  bool in_flight[2] = {false, false};
  int mirrors = 1, cur = 0, next = 0;
  size_t cap = 0;
  DmvWork* work = nullptr;
  // (mirrors_: 0 = device only; events: an event per mirror, recorded behind every upload)
  int create(size_t bytes, int mirrors_ = 1, bool events = false) {
    mirrors = mirrors_;
    HIPCHK(hipMalloc((void**)&d, std::max<size_t>(bytes, 1)));
    for (int k = 0; k < mirrors; k++) {
      HIPCHK(hipHostMalloc((void**)&h[k], std::max<size_t>(bytes, 1), hipHostMallocDefault));
      if (events) HIPCHK(hipEventCreateWithFlags(&landed[k], hipEventDisableTiming));
    }
    cap = bytes;
    return 0;
  }
  // at least `need` bytes; growing drains the stream (kernels may still read the old buffer), frees, and allocates `want`.  What the slab held is not kept.
  int reserve(size_t need, size_t want, hipStream_t s) {
    if (need <= cap) return 0;
    HIPCHK(hipStreamSynchronize(s));
    const bool events = landed[0] != nullptr;
    release();
    return create(want, mirrors, events);
  }
  bool busy() const { return in_flight[next]; }
  int begin(hipStream_t s) {
    cur = next;
    if (in_flight[cur]) HIPCHK(landed[cur] ? hipEventSynchronize(landed[cur]) : hipStreamSynchronize(s));   // this mirror's last upload; with an event, not the stream
    in_flight[cur] = false;
    return 0;
  }
  // the host pointer and the matching device pointer of one offset
  template <class T> struct Put { T* h; T* d; };
  template <class T> Put<T> put(size_t off) const { return {host<T>(off), dev<T>(off)}; }
  template <class T> T* host(size_t off) const { return reinterpret_cast<T*>(h[cur] + off); }
  template <class T> T* dev(size_t off) const { return reinterpret_cast<T*>(d + off); }
  int upload(hipStream_t s, size_t bytes) {
    HIPCHK(hipMemcpyAsync(d, h[cur], bytes, hipMemcpyHostToDevice, s));
    if (landed[cur]) HIPCHK(hipEventRecord(landed[cur], s));
    in_flight[cur] = true;
    if (mirrors == 2) next = cur ^ 1;
    if (work) work->uploads++;
    return 0;
  }
  int download(hipStream_t s, size_t off, size_t bytes) { HIPCHK(hipMemcpyAsync(h[cur] + off, d + off, bytes, hipMemcpyDeviceToHost, s)); if (work) work->downloads++; return 0; }
  void settled() { in_flight[0] = in_flight[1] = false; }
  int wait(hipStream_t s) { HIPCHK(hipStreamSynchronize(s)); if (work) work->waits++; settled(); return 0; }
  void release() {
    for (int k = 0; k < 2; k++) { if (landed[k]) hipEventDestroy(landed[k]); if (h[k]) hipHostFree(h[k]); landed[k] = nullptr; h[k] = nullptr; }
    if (d) hipFree(d);
    d = nullptr; cap = 0; cur = next = 0;
    settled();
  }
};
#endif
