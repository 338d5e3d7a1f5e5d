// The resident state a handle carries behind dmvio_hip_initializer::resident, and the launches on it that more than one unit enqueues.  capi_init_resident.hip owns the
// state, installs it (set_resident; dmvInitResidentAdopt for capi_init_first.hip) and defines the launches; capi_init_lm.hip and capi_init_lm_batch.hip run trackFrame's LM
// loop on it (init_lm_host.hpp).  Only touched under the context's lock: every function here runs under the lock its caller holds.
#pragma once
#include <cstring>
#include "init_handle.h"
#include "init_resident_host.hpp"   // the slab's layout

// The pinned side of `st` keeps the host copy of (u, v) the range checks read.
struct DmvInitResident : DmvInitResidentLayout {
  bool live = false;
  int n = 0, levels = 0, n_listed = 0, max_parent = -1, cur = 0;   // cur: which of the two JbBuffers is JbBuffer, the other being JbBuffer_new
  bool has_parent = false;
  DmvSlab st;       // the point set
  DmvSlab io;       // [what a calc downloads: IN_PART sums, 3 calcEC sums, the outside count | partials of the evaluation | partials of calcEC]
  DmvWork work;
  bool work_closed = true;
  size_t lds_limit = 0;
  float* f(size_t off) const { return st.dev<float>(off); }
  int* i(size_t off) const { return st.dev<int>(off); }
  unsigned char* b(size_t off) const { return st.dev<unsigned char>(off); }
  void put(size_t off, const void* src, size_t bytes) const { if (bytes) memcpy(st.host<char>(off), src, bytes); }   // into the pinned side
};
enum { RES_OUT_FLOATS = 128, RES_EC = dmv::IN_PART, RES_COUNT = dmv::IN_PART + 3, RES_DOWN = dmv::IN_PART + 4 };
// bytes of LDS the ordered sweeps need for n points: iR and isGood of the level
static inline size_t resSweepLds(int n) { return (5 * (size_t)n + 3) & ~(size_t)3; }
// the grid of a per-point pass: a thread a point
static inline dim3 resGrid(int n) { return dim3((unsigned)((n + 255) / 256)); }

// The evaluation reads the image around every good point without a test, so a point set is held to [2, wl - 3) x [2, hl - 3) of its wl x hl level.  The host copy of
// (u, v) says whether ANY point, good or not, lies outside: the first such point, or -1.  isGood lives on the device: resCountOutside.
static inline int resFirstOutside(const DmvInitResident* R, int wl, int hl) {
  const float *hu = R->st.host<float>(R->o_u), *hv = R->st.host<float>(R->o_v);
  const float umax = (float)(wl - 3), vmax = (float)(hl - 3);
  for (int i = 0; i < R->n; i++)
    if (!(hu[i] >= 2.0f && hu[i] < umax && hv[i] >= 2.0f && hv[i] < vmax)) return i;
  return -1;
}

// ---- capi_init_resident.hip: the passes the host-driven entry points and the LM unit both enqueue, on stream s.  Each launch is counted into `work` (NULL: nowhere); a level
// without points launches nothing.
// propagateDown (:749-777) into R from U, the level above
int resPropagateDown(DmvInitResident* R, const DmvInitResident* U, hipStream_t s, DmvWork* work);
// propagateUp (:708-747) into R from Lo, the level below
int resPropagateUp(DmvInitResident* R, const DmvInitResident* Lo, hipStream_t s, DmvWork* work);
// the GOOD points of R outside the margin, counted on the device: a memset, a launch, a download and a wait of their own, all counted into `work` or none of them
int resCountOutside(DmvInitResident* R, int wl, int hl, hipStream_t s, DmvWork* work, int* outside);
