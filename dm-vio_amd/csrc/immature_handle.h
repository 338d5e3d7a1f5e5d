// the immature-point handle, shared by capi_immature.hip (construction, tracing, optimisation) and capi_activate.hip (activation, removal)
#pragma once
#include <algorithm>
#include <vector>
#include "internal.h"
#include "immature_types.hpp"

struct dmvio_hip_immature {
  dmvio_hip_ctx* ctx = nullptr;
  int capacity = 0, n = 0, max_tag = -1;   // max_tag: largest host_tag among the points (validated against the tables of a call)
  dmv::ImmaturePts P{};
  dmv::ImmaturePts P2{};       // the arrays dmvio_hip_immature_remove_marked compacts into; swapped with P afterwards
  dmv::ImmatureSettings S;
  float* d_tables = nullptr;   // [KRKi 9H | Kt 3H | aff 2H], H <= 64
  float* h_tables = nullptr;   // pinned
  int* h_counts = nullptr;     // pinned, 16 + 64 ints: status histogram of the last traceNewCoarse (k_status_hist), counters of the activation and removal kernels
  int* d_uv_stage = nullptr;   // 2 x capacity ints
  float* d_opt_tables = nullptr;   // [R 9 F*F | t 3 F*F | aff 2 F*F], F <= 8
  float* h_opt_tables = nullptr;
  int *d_result = nullptr, *d_res_state = nullptr;
  float* d_idepth = nullptr;
  unsigned char* d_select = nullptr;
  // activation (capi_activate.hip)
  int* d_decision = nullptr;        // per point: 0 stays, 1 selected, 2 deleted (3 inside a call: passed the prefilter, waits for the ordered walk)
  unsigned char* d_mark = nullptr;  // per point: leaves the handle at the next remove_marked
  unsigned char* d_act_select = nullptr;   // per point: decision == 1, the mask optimize_selected hands to the optimisation kernel
  int* d_order = nullptr;           // toOptimize[k] -> handle index
  int* d_surv = nullptr;            // the ordered walk's list
  int* d_pidx = nullptr;            // projected level-1 pixel u + w1*v
  float *d_frac = nullptr, *d_thr = nullptr;   // ptp[0] - floorf(ptp[0]); minActDist * my_type
  int *d_newidx = nullptr, *d_holes = nullptr; // removal plan
  int* d_act_counts = nullptr;      // 8 + 64 ints
  int* d_gather_i = nullptr;        // optimize_selected, toOptimize order: result | host tag | res_state 8
  float* d_gather_f = nullptr;      //   idepth | u | v | my_type | idepth_min | idepth_max | energyTH | color 8 | weights 8
  int n_selected = 0, n_activated = 0, last_F = 0;
  bool have_selection = false, force_global_walk = false;
  long long act_stats[4] = {0, 0, 0, 0};
  DmvBounce bounce;            // caller-owned arrays cross PCIe through the library's pinned memory (internal.h)
  std::vector<void*> allocs;
};

#define IMM_READY(m) do { if (!(m)) return failmsg("null immature handle"); HIPCHK(hipSetDevice((m)->ctx->device)); } while (0)
enum { IMM_MAX_HOSTS = 64 };

template <class T>
static int ialloc(dmvio_hip_immature* m, T** p, size_t n) {
  HIPCHK(hipMalloc((void**)p, sizeof(T) * std::max<size_t>(n, 1)));
  HIPCHK(hipMemset(*p, 0, sizeof(T) * std::max<size_t>(n, 1)));
  // hipMemset clears on the NULL stream without blocking the host, and the handle's stream is non-blocking: without this wait an upload enqueued next could
  // land before the clear does (seen with two processes sharing a GPU)
  HIPCHK(hipStreamSynchronize(nullptr));
  m->allocs.push_back(*p);
  return 0;
}
static int dmv_immature_alloc_pts(dmvio_hip_immature* m, dmv::ImmaturePts& P) {
  const size_t c = m->capacity;
  return ialloc(m, &P.u, c) || ialloc(m, &P.v, c) || ialloc(m, &P.host, c) || ialloc(m, &P.color, 8 * c) || ialloc(m, &P.weights, 8 * c) || ialloc(m, &P.gradH, 4 * c) ||
         ialloc(m, &P.energyTH, c) || ialloc(m, &P.idepth_min, c) || ialloc(m, &P.idepth_max, c) || ialloc(m, &P.quality, c) || ialloc(m, &P.lastTraceUV, 2 * c) ||
         ialloc(m, &P.lastTracePixelInterval, c) || ialloc(m, &P.lastTraceStatus, c) || ialloc(m, &P.my_type, c);
}

// traceNewCoarse of W windows per call (capi_immature.hip).  One slab per call: [TraceWin x W | every window's table rows KRKi 9H, Kt 3H, aff 2H], filled in a pinned
// mirror and uploaded in one copy.  A call that does not wait leaves that copy in flight, so the slab has two mirrors and an event behind each upload; before a mirror
// is filled again only its own event is waited for (the upload before the previous one), never the stream (DmvSlab::begin, batch_slab.hpp).
struct dmvio_hip_trace_batch {
  dmvio_hip_ctx* ctx = nullptr;
  int max_windows = 0;
  DmvSlab slab;                // max_windows records + max_windows x 64 x 14 floats (dmvTraceSlabBytes)
  int* h_counts = nullptr;     // pinned, 6 x max_windows: k_status_hist_b stores straight into it
};

// per-host tables hostToNew: KRKi = Kleft * R * K0^-1, Kt = Kleft * t (floats, the reference's product order; FullSystem.cpp:548-552 with Kleft = K0,
// CoarseTracker.cpp:949-951 with Kleft = K[1]); K0 from fxfycxcy, its inverse as Eigen's 3x3 cofactor inverse
void dmv_host_tables(const float Kleft[9], const double fxfycxcy[4], const double new_w2c7[7], int n_hosts, const double* host_c2w7, float* KRKi9, float* Kt3);
// the selector's status map of its last call (w*h bytes on the device; capi_select.hip)
const unsigned char* dmv_selector_map(dmvio_hip_pixel_selector* s);
// dmvio_hip_immature_optimize up to and including the kernel, for a mask that is already on the device (d_mask per point; results stay in d_result / d_idepth /
// d_res_state).  The caller holds the context's mutex.  stream_idle: the caller has waited for the stream since this handle's tables were last uploaded (a batch of
// handles waits once for all of them); otherwise the call waits itself before it rewrites them.
int dmv_immature_optimize_launch_locked(dmvio_hip_immature* m, int F, const int* frame_slots, const double* w2c7, const double* aff2, const float* exposure,
                                        const double fxfycxcy[4], const unsigned char* d_mask, int minObs, bool stream_idle = false);
