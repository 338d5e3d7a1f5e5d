// C ABI of point activation (include/dmvio_hip.h): CoarseDistanceMap, the candidate loop and the compaction of FullSystem::activatePointsMT.
#include <vector>
#include <cmath>
#include <cstring>
#include <algorithm>
#include "../../include/dmvio_hip.h"
#include "internal.h"
#include "immature_handle.h"
#include "activate_batch_kernels.hpp"

using namespace dmv;

struct dmvio_hip_distance_map {
  dmvio_hip_ctx* ctx = nullptr;
  DmGeom G{};
  int map_bytes = 0;                 // w1*h1 rounded up to 16
  unsigned char* d_map = nullptr;
  float* d_tables = nullptr;         // [KRKi 9*64 | Kt 3*64] of make, the same of select_for_activation behind it
  unsigned char* d_flagged = nullptr;
  int cap = 0;                       // active points the staging arrays hold
  int* d_host = nullptr;
  float* d_uvi = nullptr;            // u | v | idepth
  bool made = false;
  DmvBounce bounce;
};
enum { DM_TAB = 12 * IMM_MAX_HOSTS };

#define DM_READY(d) do { if (!(d)) return failmsg("null distance map handle"); HIPCHK(hipSetDevice((d)->ctx->device)); } while (0)

static int dmUploadTables(dmvio_hip_distance_map* dm, int which, int n_hosts, const float* KRKi9, const float* Kt3, hipStream_t st) {
  float* t = dm->d_tables + which * DM_TAB;
  HIPCHK(dm->bounce.h2d(t, KRKi9, sizeof(float) * 9 * n_hosts, st));
  HIPCHK(dm->bounce.h2d(t + 9 * IMM_MAX_HOSTS, Kt3, sizeof(float) * 3 * n_hosts, st));
  return 0;
}
static size_t walkLds(bool lds, int map_bytes) { return (lds ? (size_t)map_bytes : 0) + sizeof(int) * 2 * ACT_LIST; }
static int allowBigLds() {
  static bool done = false;
  if (!done) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_act_walk<true>), hipFuncAttributeMaxDynamicSharedMemorySize, ACT_LDS_BUDGET - 1024));
    done = true;
  }
  return 0;
}
static int allowBigLdsBatch() {
  static bool done = false;
  if (!done) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_act_ordered_walk_b<true>), hipFuncAttributeMaxDynamicSharedMemorySize, ACT_LDS_BUDGET - 1024));
    done = true;
  }
  return 0;
}

extern "C" {

dmvio_hip_distance_map* dmvio_hip_distance_map_create(dmvio_hip_ctx* ctx) {
  if (!ctx) { failmsg("distance_map_create: null context"); return nullptr; }
  if ((ctx->w >> 1) < 3 || (ctx->h >> 1) < 3 || (ctx->w >> 1) > 0xffff || (ctx->h >> 1) > 0x7fff) { failmsg("distance_map_create: image size out of range"); return nullptr; }
  HIPCHKP(hipSetDevice(ctx->device));
  dmvio_hip_distance_map* dm = new dmvio_hip_distance_map();
  dm->ctx = ctx;
  dm->G.w1 = ctx->w >> 1; dm->G.h1 = ctx->h >> 1;   // CoarseDistanceMap::makeK, CoarseTracker.cpp:1098-1099
  dm->map_bytes = (dm->G.w1 * dm->G.h1 + 15) & ~15;
  if (hipMalloc((void**)&dm->d_map, dm->map_bytes) != hipSuccess || hipMalloc((void**)&dm->d_tables, sizeof(float) * 2 * DM_TAB) != hipSuccess ||
      hipMalloc((void**)&dm->d_flagged, IMM_MAX_HOSTS) != hipSuccess || hipMemset(dm->d_map, DM_FAR, dm->map_bytes) != hipSuccess ||
      hipMemset(dm->d_tables, 0, sizeof(float) * 2 * DM_TAB) != hipSuccess || hipMemset(dm->d_flagged, 0, IMM_MAX_HOSTS) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess) {
    failmsg("distance_map_create: allocation failed");
    if (dm->d_map) hipFree(dm->d_map);
    if (dm->d_tables) hipFree(dm->d_tables);
    if (dm->d_flagged) hipFree(dm->d_flagged);
    delete dm;
    return nullptr;
  }
  return dm;
}
void dmvio_hip_distance_map_destroy(dmvio_hip_distance_map* dm) {
  if (!dm) return;
  hipSetDevice(dm->ctx->device);
  hipStreamSynchronize(dm->ctx->stream);
  hipFree(dm->d_map); hipFree(dm->d_tables); hipFree(dm->d_flagged);
  if (dm->d_host) hipFree(dm->d_host);
  if (dm->d_uvi) hipFree(dm->d_uvi);
  dm->bounce.release();
  delete dm;
}
int dmvio_hip_distance_map_size(dmvio_hip_distance_map* dm, int* w1, int* h1) {
  if (!dm) return failmsg("null distance map handle");
  if (w1) *w1 = dm->G.w1;
  if (h1) *h1 = dm->G.h1;
  return dm->G.w1 * dm->G.h1;
}

int dmvio_hip_distance_map_tables_from_poses(const double new_w2c7[7], int n_hosts, const double* host_c2w7, const double fxfycxcy[4], float* KRKi9, float* Kt3) {
  if (!new_w2c7 || !host_c2w7 || !fxfycxcy || !KRKi9 || !Kt3 || n_hosts < 1 || n_hosts > IMM_MAX_HOSTS) return failmsg("distance_map_tables_from_poses: bad argument");
  // CoarseDistanceMap::makeK (CoarseTracker.cpp:1086-1115): float members, the right-hand sides evaluated in double
  const float fx0 = (float)fxfycxcy[0], fy0 = (float)fxfycxcy[1], cx0 = (float)fxfycxcy[2], cy0 = (float)fxfycxcy[3];
  const float fx1 = (float)((double)fx0 * 0.5), fy1 = (float)((double)fy0 * 0.5);
  const float cx1 = (float)(((double)cx0 + 0.5) / 2 - 0.5), cy1 = (float)(((double)cy0 + 0.5) / 2 - 0.5);
  const float K1[9] = {fx1, 0, cx1, 0, fy1, cy1, 0, 0, 1};
  dmv_host_tables(K1, fxfycxcy, new_w2c7, n_hosts, host_c2w7, KRKi9, Kt3);
  return 0;
}

int dmvio_hip_distance_map_make(dmvio_hip_distance_map* dm, int n_hosts, const float* KRKi9, const float* Kt3, int n_points, const int* host_tag, const float* u, const float* v,
                                const float* idepth_scaled) {
  DM_READY(dm);
  dmvio_hip_ctx* c = dm->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (n_hosts < 1 || n_hosts > IMM_MAX_HOSTS || !KRKi9 || !Kt3 || n_points < 0 || (n_points > 0 && (!host_tag || !u || !v || !idepth_scaled)))
    return failmsg("distance_map_make: bad argument");
  for (int i = 0; i < n_points; i++)
    if (host_tag[i] < 0 || host_tag[i] >= n_hosts) return failmsg("distance_map_make: a point's host_tag has no table row");
  hipStream_t st = c->stream;
  if (n_points > dm->cap) {
    HIPCHK(hipStreamSynchronize(st));
    if (dm->d_host) HIPCHK(hipFree(dm->d_host));
    if (dm->d_uvi) HIPCHK(hipFree(dm->d_uvi));
    dm->d_host = nullptr; dm->d_uvi = nullptr; dm->cap = 0;
    const int cap = std::max(4096, n_points + n_points / 2);
    HIPCHK(hipMalloc((void**)&dm->d_host, sizeof(int) * cap));
    HIPCHK(hipMalloc((void**)&dm->d_uvi, sizeof(float) * 3 * cap));
    dm->cap = cap;
  }
  if (int r = dmUploadTables(dm, 0, n_hosts, KRKi9, Kt3, st)) return r;
  HIPCHK(hipMemsetAsync(dm->d_map, DM_FAR, dm->map_bytes, st));
  if (n_points > 0) {
    const size_t n = n_points;
    HIPCHK(dm->bounce.h2d(dm->d_host, host_tag, sizeof(int) * n, st));
    HIPCHK(dm->bounce.h2d(dm->d_uvi, u, sizeof(float) * n, st));
    HIPCHK(dm->bounce.h2d(dm->d_uvi + dm->cap, v, sizeof(float) * n, st));
    HIPCHK(dm->bounce.h2d(dm->d_uvi + 2 * (size_t)dm->cap, idepth_scaled, sizeof(float) * n, st));
    hipLaunchKernelGGL(k_dm_seed, dim3((n_points + 255) / 256), dim3(256), 0, st, n_points, (const int*)dm->d_host, (const float*)dm->d_uvi, (const float*)(dm->d_uvi + dm->cap),
                       (const float*)(dm->d_uvi + 2 * (size_t)dm->cap), (const float*)dm->d_tables, (const float*)(dm->d_tables + 9 * IMM_MAX_HOSTS), dm->G, dm->d_map);
    const int npix = dm->G.w1 * dm->G.h1;
    for (int k = 1; k < DM_STEPS; k++) hipLaunchKernelGGL(k_dm_grow, dim3((npix + 255) / 256), dim3(256), 0, st, dm->d_map, dm->G, k);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(dm->bounce.finish(st));   // the staged inputs may be reused by the caller's next call
  dm->made = true;
  return 0;
}

int dmvio_hip_distance_map_add(dmvio_hip_distance_map* dm, int u, int v) {
  DM_READY(dm);
  dmvio_hip_ctx* c = dm->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (u < 0 || v < 0 || u >= dm->G.w1 || v >= dm->G.h1) return failmsg("distance_map_add: pixel outside the level-1 image");
  hipLaunchKernelGGL(k_dm_add, dim3(1), dim3(ACT_THREADS), walkLds(false, 0), c->stream, dm->d_map, dm->G, u, v);
  HIPCHK(hipGetLastError());
  return 0;
}

int dmvio_hip_distance_map_get(dmvio_hip_distance_map* dm, float* map) {
  DM_READY(dm);
  dmvio_hip_ctx* c = dm->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!map) return failmsg("distance_map_get: map is NULL");
  const int npix = dm->G.w1 * dm->G.h1;
  size_t off;
  HIPCHK(dm->bounce.reserve((size_t)npix, c->stream, &off));
  HIPCHK(hipMemcpyAsync(dm->bounce.h + off, dm->d_map, (size_t)npix, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(dm->bounce.finish(c->stream));
  const unsigned char* b = reinterpret_cast<const unsigned char*>(dm->bounce.h + off);
  for (int i = 0; i < npix; i++) map[i] = b[i] == DM_FAR ? 1000.f : (float)b[i];
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------------
int dmvio_hip_immature_set_types(dmvio_hip_immature* m, const float* my_type) {
  IMM_READY(m);
  if (!my_type) return failmsg("immature_set_types: my_type is NULL");
  HIPCHK(m->bounce.h2d(m->P.my_type, my_type, sizeof(float) * (size_t)m->n, m->ctx->stream));
  HIPCHK(m->bounce.finish(m->ctx->stream));
  return 0;
}
int dmvio_hip_immature_get_types(dmvio_hip_immature* m, float* my_type) {
  IMM_READY(m);
  if (!my_type) return failmsg("immature_get_types: my_type is NULL");
  HIPCHK(m->bounce.d2h(my_type, m->P.my_type, sizeof(float) * (size_t)m->n, m->ctx->stream));
  HIPCHK(m->bounce.finish(m->ctx->stream));
  return 0;
}
int dmvio_hip_immature_set_last_trace(dmvio_hip_immature* m, const float* lastTraceUV2, const float* lastTracePixelInterval) {
  IMM_READY(m);
  hipStream_t s = m->ctx->stream;
  if (lastTraceUV2) HIPCHK(m->bounce.h2d(m->P.lastTraceUV, lastTraceUV2, sizeof(float) * 2 * (size_t)m->n, s));
  if (lastTracePixelInterval) HIPCHK(m->bounce.h2d(m->P.lastTracePixelInterval, lastTracePixelInterval, sizeof(float) * (size_t)m->n, s));
  HIPCHK(m->bounce.finish(s));
  return 0;
}
int dmvio_hip_immature_set_activation_walk(dmvio_hip_immature* m, int global_memory) {
  if (!m) return failmsg("null immature handle");
  m->force_global_walk = global_memory != 0;
  return 0;
}

int dmvio_hip_immature_select_for_activation(dmvio_hip_immature* m, dmvio_hip_distance_map* dm, int n_hosts, const float* KRKi9, const float* Kt3,
                                             const unsigned char* host_flagged, int newest_tag, float minActDist, float minTraceQuality, int* n_selected, int* n_deleted) {
  IMM_READY(m);
  dmvio_hip_ctx* c = m->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!dm || dm->ctx != c) return failmsg("immature_select_for_activation: the distance map is NULL or belongs to another context");
  if (!dm->made) return failmsg("immature_select_for_activation: the distance map has not been made (dmvio_hip_distance_map_make)");
  if (n_hosts < 1 || n_hosts > IMM_MAX_HOSTS || !KRKi9 || !Kt3 || !host_flagged) return failmsg("immature_select_for_activation: bad argument");
  if (m->max_tag >= n_hosts) return failmsg("immature_select_for_activation: a point's host_tag has no table row (host_tag >= n_hosts)");
  hipStream_t st = c->stream;
  m->have_selection = false; m->n_selected = m->n_activated = 0;
  for (int k = 0; k < 4; k++) m->act_stats[k] = 0;
  if (n_selected) *n_selected = 0;
  if (n_deleted) *n_deleted = 0;
  if (m->n > 0) {
    if (int r = dmUploadTables(dm, 1, n_hosts, KRKi9, Kt3, st)) return r;
    HIPCHK(dm->bounce.h2d(dm->d_flagged, host_flagged, n_hosts, st));
    HIPCHK(hipMemsetAsync(m->d_act_counts, 0, sizeof(int) * 8, st));
    m->P.n = m->n;
    ActArgs A;
    A.n = m->n; A.n_hosts = n_hosts; A.newest_tag = newest_tag; A.minActDist = minActDist; A.minTraceQuality = minTraceQuality;
    A.KRKi = dm->d_tables + DM_TAB; A.Kt = dm->d_tables + DM_TAB + 9 * IMM_MAX_HOSTS; A.flagged = dm->d_flagged;
    hipLaunchKernelGGL(k_act_classify, dim3((m->n + 255) / 256), dim3(256), 0, st, m->P, A, dm->G, (const unsigned char*)dm->d_map, m->d_decision, m->d_pidx, m->d_frac,
                       m->d_thr, m->d_act_counts);
    const bool lds = !m->force_global_walk && walkLds(true, dm->map_bytes) + 1024 <= (size_t)ACT_LDS_BUDGET;
    if (lds) {
      if (int r = allowBigLds()) return r;
      hipLaunchKernelGGL(k_act_walk<true>, dim3(1), dim3(ACT_THREADS), walkLds(true, dm->map_bytes), st, m->P, A, dm->G, dm->d_map, dm->map_bytes, m->d_decision,
                         (const int*)m->d_pidx, (const float*)m->d_frac, (const float*)m->d_thr, m->d_surv, m->d_order, m->d_act_select, m->d_mark, m->d_act_counts);
    } else {
      hipLaunchKernelGGL(k_act_walk<false>, dim3(1), dim3(ACT_THREADS), walkLds(false, 0), st, m->P, A, dm->G, dm->d_map, dm->map_bytes, m->d_decision,
                         (const int*)m->d_pidx, (const float*)m->d_frac, (const float*)m->d_thr, m->d_surv, m->d_order, m->d_act_select, m->d_mark, m->d_act_counts);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(m->h_counts + 8, m->d_act_counts, sizeof(int) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(dm->bounce.finish(st));
    const int* hc = m->h_counts + 8;
    m->act_stats[0] = hc[ACTC_CLASSIFIED]; m->act_stats[1] = hc[ACTC_SURVIVORS]; m->act_stats[2] = hc[ACTC_ACCEPTED]; m->act_stats[3] = hc[ACTC_DELETED];
    m->n_selected = hc[ACTC_ACCEPTED];
  }
  m->have_selection = true;
  if (n_selected) *n_selected = m->n_selected;
  if (n_deleted) *n_deleted = (int)m->act_stats[3];
  return 0;
}

int dmvio_hip_immature_get_activation_stats(dmvio_hip_immature* m, long long stats4[4]) {
  if (!m || !stats4) return failmsg("immature_get_activation_stats: null argument");
  for (int k = 0; k < 4; k++) stats4[k] = m->act_stats[k];
  return 0;
}

int dmvio_hip_immature_get_activation(dmvio_hip_immature* m, int* decision, int* order) {
  IMM_READY(m);
  if (!m->have_selection) return failmsg("immature_get_activation: no selection (dmvio_hip_immature_select_for_activation)");
  hipStream_t st = m->ctx->stream;
  if (decision) HIPCHK(m->bounce.d2h(decision, m->d_decision, sizeof(int) * (size_t)m->n, st));
  if (order) HIPCHK(m->bounce.d2h(order, m->d_order, sizeof(int) * (size_t)m->n_selected, st));
  HIPCHK(m->bounce.finish(st));
  return m->n_selected;
}
int dmvio_hip_immature_get_marks(dmvio_hip_immature* m, unsigned char* mark) {
  IMM_READY(m);
  if (!mark) return failmsg("immature_get_marks: mark is NULL");
  if (!m->have_selection) { memset(mark, 0, (size_t)m->n); return 0; }
  HIPCHK(m->bounce.d2h(mark, m->d_mark, (size_t)m->n, m->ctx->stream));
  HIPCHK(m->bounce.finish(m->ctx->stream));
  return 0;
}

int dmvio_hip_immature_optimize_selected(dmvio_hip_immature* m, int F, const int* frame_slots, const double* w2c7, const double* aff2, const float* exposure,
                                         const double fxfycxcy[4], int minObs, int* result, float* idepth, int* res_state) {
  IMM_READY(m);
  dmvio_hip_ctx* c = m->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!m->have_selection) return failmsg("immature_optimize_selected: no selection (dmvio_hip_immature_select_for_activation)");
  m->n_activated = 0; m->last_F = F;
  const int ns = m->n_selected;
  if (ns == 0) return 0;
  if (int r = dmv_immature_optimize_launch_locked(m, F, frame_slots, w2c7, aff2, exposure, fxfycxcy, m->d_act_select, minObs)) return r;
  hipStream_t st = c->stream;
  HIPCHK(hipMemsetAsync(m->d_act_counts + ACTC_ACTIVATED, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_act_gather, dim3((ns + 255) / 256), dim3(256), 0, st, m->P, ns, F, (const int*)m->d_order, (const int*)m->d_result, (const float*)m->d_idepth,
                     (const int*)m->d_res_state, m->d_mark, m->d_gather_i, m->d_gather_f, m->d_act_counts);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(m->h_counts + 8, m->d_act_counts, sizeof(int) * 8, hipMemcpyDeviceToHost, st));
  if (result) HIPCHK(m->bounce.d2h(result, m->d_gather_i, sizeof(int) * (size_t)ns, st));
  if (idepth) HIPCHK(m->bounce.d2h(idepth, m->d_gather_f, sizeof(float) * (size_t)ns, st));
  std::vector<int> rs8;
  if (res_state) { rs8.resize(8 * (size_t)ns); HIPCHK(m->bounce.d2h(rs8.data(), m->d_gather_i + 2 * (size_t)ns, sizeof(int) * 8 * (size_t)ns, st)); }
  HIPCHK(m->bounce.finish(st));
  if (res_state) for (int k = 0; k < ns; k++) for (int t = 0; t < F; t++) res_state[(size_t)k * F + t] = rs8[8 * (size_t)k + t];
  m->n_activated = m->h_counts[8 + ACTC_ACTIVATED];
  return m->n_activated;
}

int dmvio_hip_immature_mark_optimized(dmvio_hip_immature* m, const int* result) {
  IMM_READY(m);
  dmvio_hip_ctx* c = m->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!m->have_selection) return failmsg("immature_mark_optimized: no selection (dmvio_hip_immature_select_for_activation)");
  if (m->n_selected == 0) return 0;
  if (!result) return failmsg("immature_mark_optimized: result is NULL");
  m->P.n = m->n;
  HIPCHK(m->bounce.h2d(m->d_result, result, sizeof(int) * (size_t)m->n_selected, c->stream));
  hipLaunchKernelGGL(k_act_mark_results, dim3((m->n_selected + 255) / 256), dim3(256), 0, c->stream, m->P, m->n_selected, (const int*)m->d_order, (const int*)m->d_result,
                     m->d_mark);
  HIPCHK(hipGetLastError());
  HIPCHK(m->bounce.finish(c->stream));
  return 0;
}

int dmvio_hip_immature_get_activated(dmvio_hip_immature* m, int* host_tag, float* u, float* v, float* my_type, float* idepth_min, float* idepth_max, float* color8,
                                     float* weights8, float* energyTH, float* idepth, int* res_state) {
  IMM_READY(m);
  if (!m->have_selection) return failmsg("immature_get_activated: no selection");
  const size_t ns = m->n_selected;
  if (ns == 0 || m->n_activated == 0) return 0;
  const int F = m->last_F;
  std::vector<int> gi(10 * ns);
  std::vector<float> gf(23 * ns);
  hipStream_t st = m->ctx->stream;
  HIPCHK(m->bounce.d2h(gi.data(), m->d_gather_i, sizeof(int) * 10 * ns, st));
  HIPCHK(m->bounce.d2h(gf.data(), m->d_gather_f, sizeof(float) * 23 * ns, st));
  HIPCHK(m->bounce.finish(st));
  size_t a = 0;
  for (size_t k = 0; k < ns; k++) {
    if (gi[k] != 1) continue;
    if (host_tag) host_tag[a] = gi[ns + k];
    if (idepth) idepth[a] = gf[k];
    if (u) u[a] = gf[ns + k];
    if (v) v[a] = gf[2 * ns + k];
    if (my_type) my_type[a] = gf[3 * ns + k];
    if (idepth_min) idepth_min[a] = gf[4 * ns + k];
    if (idepth_max) idepth_max[a] = gf[5 * ns + k];
    if (energyTH) energyTH[a] = gf[6 * ns + k];
    if (color8) memcpy(color8 + 8 * a, &gf[7 * ns + 8 * k], sizeof(float) * 8);
    if (weights8) memcpy(weights8 + 8 * a, &gf[15 * ns + 8 * k], sizeof(float) * 8);
    if (res_state) for (int t = 0; t < F; t++) res_state[a * F + t] = gi[2 * ns + 8 * k + t];
    a++;
  }
  return (int)a;
}

static int removePlanned(dmvio_hip_immature* m, int drop_tag) {
  dmvio_hip_ctx* c = m->ctx;
  hipStream_t st = c->stream;
  const int n_tags = m->max_tag + 1;
  hipLaunchKernelGGL(k_rm_plan, dim3(1), dim3(ACT_THREADS), 0, st, (const int*)m->P.host, (const unsigned char*)m->d_mark, m->n, n_tags, m->d_newidx, m->d_holes, m->d_act_counts);
  m->P.n = m->n; m->P2.n = m->n;
  hipLaunchKernelGGL(k_rm_apply, dim3((m->n + 255) / 256), dim3(256), 0, st, m->P, m->P2, m->n, (const int*)m->d_newidx, drop_tag);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(m->h_counts + 8, m->d_act_counts, sizeof(int) * (8 + IMM_MAX_HOSTS), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::swap(m->P, m->P2);
  m->n = m->h_counts[8 + ACTC_NEW_N];
  int mt = -1;
  for (int t = 0; t < n_tags; t++)
    if (m->h_counts[8 + ACTC_TAGS + t] > 0) mt = (drop_tag >= 0 && t > drop_tag) ? t - 1 : t;
  m->max_tag = mt;
  m->P.n = m->n;
  m->have_selection = false; m->n_selected = m->n_activated = 0;
  return m->n;
}

int dmvio_hip_immature_remove_marked(dmvio_hip_immature* m) {
  IMM_READY(m);
  std::lock_guard<std::mutex> lk(m->ctx->mu);
  if (!m->have_selection) return failmsg("immature_remove_marked: no marks (dmvio_hip_immature_select_for_activation)");
  if (m->n == 0) { m->have_selection = false; return 0; }
  return removePlanned(m, -1);
}

int dmvio_hip_immature_remove_host(dmvio_hip_immature* m, int tag) {
  IMM_READY(m);
  std::lock_guard<std::mutex> lk(m->ctx->mu);
  if (tag < 0 || tag >= IMM_MAX_HOSTS) return failmsg("immature_remove_host: tag out of range");
  if (m->n == 0) return 0;
  m->P.n = m->n;
  hipLaunchKernelGGL(k_rm_mark_host, dim3((m->n + 255) / 256), dim3(256), 0, m->ctx->stream, m->P, m->n, tag, m->d_mark);
  if (tag > m->max_tag) { /* nothing to delete; tags stay */ }
  return removePlanned(m, tag);
}

// the sparsity controller of FullSystem::activatePointsMT (FullSystem.cpp:608-627): currentMinActDist is a float, the literals are doubles
float dmvio_hip_min_act_dist_update(float cur, int nPoints, float desiredDensity) {
  if (nPoints < desiredDensity * 0.66) cur -= 0.8;
  if (nPoints < desiredDensity * 0.8) cur -= 0.5;
  else if (nPoints < desiredDensity * 0.9) cur -= 0.2;
  else if (nPoints < desiredDensity) cur -= 0.1;
  if (nPoints > desiredDensity * 1.5) cur += 0.8;
  if (nPoints > desiredDensity * 1.3) cur += 0.5;
  if (nPoints > desiredDensity * 1.15) cur += 0.2;
  if (nPoints > desiredDensity) cur += 0.1;
  if (cur < 0) cur = 0;
  if (cur > 4) cur = 4;
  return cur;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------------ W windows per call
// One slab per call, written in pinned memory and uploaded in one copy: [ActWin x W | what the call's kernels read of the caller's arrays (tables, flags, active points)].
// The counters of all windows live in one slab of the batch and come back in one copy; a call waits for the stream once, at its end.
struct dmvio_hip_activation_batch {
  dmvio_hip_ctx* ctx = nullptr;
  int max_windows = 0;
  DmvSlab slab;     // grown to a call's need (batch_slab.hpp)
  DmvSlab counts;   // max_windows x ACT_COUNTS ints
};
enum { ACT_COUNTS = 8 + IMM_MAX_HOSTS };

// the slab holds at least `bytes` (one and a half times the need where it grows) and its pinned side is free to write
static int batchBegin(dmvio_hip_activation_batch* b, size_t bytes) {
  if (int r = b->slab.reserve(bytes, bytes + bytes / 2, b->ctx->stream)) return r;
  return b->slab.begin(b->ctx->stream);
}
// the part of a window's record that is the same in every call: the handle's arrays
static void recordOf(ActWin& R, dmvio_hip_activation_batch* b, int w, dmvio_hip_immature* m, dmvio_hip_distance_map* dm) {
  memset(&R, 0, sizeof(R));
  if (m) {
    R.P = m->P; R.P2 = m->P2; R.P.n = R.P2.n = m->n;
    R.n = m->n; R.n_sel = m->n_selected; R.n_tags = m->max_tag + 1;
    R.decision = m->d_decision; R.pidx = m->d_pidx; R.frac = m->d_frac; R.thr = m->d_thr; R.surv = m->d_surv; R.order = m->d_order; R.select = m->d_act_select;
    R.mark = m->d_mark; R.newidx = m->d_newidx; R.holes = m->d_holes;
    R.result = m->d_result; R.idepth = m->d_idepth; R.res_state = m->d_res_state; R.gather_i = m->d_gather_i; R.gather_f = m->d_gather_f;
  }
  if (dm) { R.map = dm->d_map; R.map_bytes = dm->map_bytes; }
  R.counts = b->counts.dev<int>(0) + (size_t)w * ACT_COUNTS;
}
static int maxOf(const std::vector<int>& v) { int m = 0; for (int x : v) m = std::max(m, x); return m; }

extern "C" {

dmvio_hip_activation_batch* dmvio_hip_activation_batch_create(dmvio_hip_ctx* ctx, int max_windows) {
  if (!ctx) { failmsg("activation_batch_create: null context"); return nullptr; }
  if (max_windows < 1 || max_windows > 65535) { failmsg("activation_batch_create: max_windows out of range (1..65535)"); return nullptr; }
  HIPCHKP(hipSetDevice(ctx->device));
  dmvio_hip_activation_batch* b = new dmvio_hip_activation_batch();
  b->ctx = ctx; b->max_windows = max_windows;
  if (b->counts.create(sizeof(int) * ACT_COUNTS * (size_t)max_windows)) {
    failmsg("activation_batch_create: allocation failed");
    b->counts.release();
    delete b;
    return nullptr;
  }
  return b;
}
void dmvio_hip_activation_batch_destroy(dmvio_hip_activation_batch* b) {
  if (!b) return;
  hipSetDevice(b->ctx->device);
  hipStreamSynchronize(b->ctx->stream);
  b->slab.release(); b->counts.release();
  delete b;
}

int dmvio_hip_distance_map_make_batch(dmvio_hip_activation_batch* b, int W, dmvio_hip_activation_window* win) {
  if (int r = dmvBatchHead(b, W, b ? b->max_windows : 0, win, "distance_map_make_batch")) return r;
  if (W == 0) return 0;
  dmvio_hip_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  // every refusal before anything is enqueued or any handle touched
  const int rep = dmvFirstRepeated(win, W, &dmvio_hip_activation_window::dm);
  DmvCursor L; L.take<ActWin>(W);   // [ActWin x W | per window: KRKi 9H, Kt 3H | host tag, u, v, idepth of its active points]
  std::vector<size_t> tabOff(W), actOff(W);
  for (int w = 0; w < W; w++) {
    const dmvio_hip_activation_window& V = win[w];
    if (!V.dm) return failmsg("distance_map_make_batch: a distance map handle is NULL");
    if (V.dm->ctx != c) return failmsg("distance_map_make_batch: a distance map belongs to another context");
    if (w == rep) return failmsg("distance_map_make_batch: a distance map appears twice");
    if (V.n_hosts < 1 || V.n_hosts > IMM_MAX_HOSTS || !V.KRKi9 || !V.Kt3 || V.n_active < 0 || (V.n_active > 0 && (!V.active_host_tag || !V.active_u || !V.active_v || !V.active_idepth)))
      return failmsg("distance_map_make_batch: bad argument (n_hosts, a table or an active-point array)");
    for (int i = 0; i < V.n_active; i++)
      if (V.active_host_tag[i] < 0 || V.active_host_tag[i] >= V.n_hosts) return failmsg("distance_map_make_batch: a point's host_tag has no table row");
    tabOff[w] = L.take<float>(12 * (size_t)V.n_hosts); actOff[w] = L.take<float>(4 * (size_t)V.n_active);
  }
  if (int r = batchBegin(b, L.bytes())) return r;
  hipStream_t st = c->stream;
  ActWin* R = b->slab.host<ActWin>(0);
  std::vector<int> na(W);
  const DmGeom G = win[0].dm->G;
  for (int w = 0; w < W; w++) {
    const dmvio_hip_activation_window& V = win[w];
    recordOf(R[w], b, w, nullptr, V.dm);
    const size_t n = V.n_active;
    R[w].n_active = na[w] = V.n_active;
    const auto t = b->slab.put<float>(tabOff[w]);
    memcpy(t.h, V.KRKi9, sizeof(float) * 9 * V.n_hosts); memcpy(t.h + 9 * V.n_hosts, V.Kt3, sizeof(float) * 3 * V.n_hosts);
    R[w].mk_KRKi = t.d; R[w].mk_Kt = t.d + 9 * V.n_hosts;
    const auto a = b->slab.put<char>(actOff[w]);
    if (n) {
      memcpy(a.h, V.active_host_tag, 4 * n); memcpy(a.h + 4 * n, V.active_u, 4 * n); memcpy(a.h + 8 * n, V.active_v, 4 * n); memcpy(a.h + 12 * n, V.active_idepth, 4 * n);
    }
    R[w].act_host = reinterpret_cast<const int*>(a.d); R[w].act_u = reinterpret_cast<const float*>(a.d + 4 * n); R[w].act_v = reinterpret_cast<const float*>(a.d + 8 * n);
    R[w].act_idepth = reinterpret_cast<const float*>(a.d + 12 * n);
  }
  if (int r = b->slab.upload(st, L.bytes())) return r;
  const ActWin* D = b->slab.dev<const ActWin>(0);
  const int npix = G.w1 * G.h1, map_bytes = win[0].dm->map_bytes, amax = maxOf(na);
  hipLaunchKernelGGL(k_dm_fill_b, dim3((map_bytes / 16 + 255) / 256, W), dim3(256), 0, st, D);
  if (amax > 0) {
    hipLaunchKernelGGL(k_dm_seed_b, dim3((amax + 255) / 256, W), dim3(256), 0, st, D, G);
    for (int k = 1; k < DM_STEPS; k++) hipLaunchKernelGGL(k_dm_grow_b, dim3((npix + 255) / 256, W), dim3(256), 0, st, D, G, k);
  }
  HIPCHK(hipGetLastError());
  if (int r = b->slab.wait(st)) return r;   // the one wait: the slab may be rewritten by the next call
  for (int w = 0; w < W; w++) win[w].dm->made = true;
  return 0;
}

int dmvio_hip_immature_select_for_activation_batch(dmvio_hip_activation_batch* b, int W, dmvio_hip_activation_window* win) {
  if (int r = dmvBatchHead(b, W, b ? b->max_windows : 0, win, "immature_select_for_activation_batch")) return r;
  if (W == 0) return 0;
  dmvio_hip_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  DmvCursor L; L.take<ActWin>(W);   // [ActWin x W | per window: KRKi 9H, Kt 3H floats, H flag bytes]
  std::vector<size_t> tabOff(W);
  bool lds = true;
  const int repImm = dmvFirstRepeated(win, W, &dmvio_hip_activation_window::imm), repDm = dmvFirstRepeated(win, W, &dmvio_hip_activation_window::dm);
  for (int w = 0; w < W; w++) {
    const dmvio_hip_activation_window& V = win[w];
    if (!V.imm || !V.dm) return failmsg("immature_select_for_activation_batch: an immature or distance map handle is NULL");
    if (V.imm->ctx != c || V.dm->ctx != c) return failmsg("immature_select_for_activation_batch: a handle belongs to another context");
    if (w == repImm || w == repDm) {
      // which of the two a walk over the earlier windows meets first: the earliest window that shares either handle, and there the immature set before the map
      int k = 0;
      while (win[k].imm != V.imm && win[k].dm != V.dm) k++;
      return failmsg(win[k].imm == V.imm ? "immature_select_for_activation_batch: an immature handle appears twice" : "immature_select_for_activation_batch: a distance map appears twice");
    }
    if (!V.dm->made) return failmsg("immature_select_for_activation_batch: a distance map has not been made (dmvio_hip_distance_map_make_batch)");
    if (V.n_hosts < 1 || V.n_hosts > IMM_MAX_HOSTS || !V.KRKi9 || !V.Kt3 || !V.host_flagged) return failmsg("immature_select_for_activation_batch: bad argument (n_hosts, a table or host_flagged)");
    if (V.imm->max_tag >= V.n_hosts) return failmsg("immature_select_for_activation_batch: a point's host_tag has no table row (host_tag >= n_hosts)");
    if (V.imm->force_global_walk || walkLds(true, V.dm->map_bytes) + 1024 > (size_t)ACT_LDS_BUDGET) lds = false;
    tabOff[w] = L.takeBytes(sizeof(float) * 12 * V.n_hosts + V.n_hosts);
  }
  if (int r = batchBegin(b, L.bytes())) return r;
  if (lds) if (int r = allowBigLdsBatch()) return r;
  hipStream_t st = c->stream;
  ActWin* R = b->slab.host<ActWin>(0);
  std::vector<int> nn(W);
  const DmGeom G = win[0].dm->G;
  for (int w = 0; w < W; w++) {
    dmvio_hip_activation_window& V = win[w];
    dmvio_hip_immature* m = V.imm;
    m->have_selection = false; m->n_selected = m->n_activated = 0;
    for (int k = 0; k < 4; k++) m->act_stats[k] = 0;
    V.n_selected = V.n_deleted = 0;
    m->P.n = m->n;
    recordOf(R[w], b, w, m, V.dm);
    nn[w] = m->n;
    const auto t = b->slab.put<float>(tabOff[w]);
    memcpy(t.h, V.KRKi9, sizeof(float) * 9 * V.n_hosts); memcpy(t.h + 9 * V.n_hosts, V.Kt3, sizeof(float) * 3 * V.n_hosts);
    memcpy(t.h + 12 * V.n_hosts, V.host_flagged, V.n_hosts);
    ActArgs& A = R[w].A;
    A.n = m->n; A.n_hosts = V.n_hosts; A.newest_tag = V.newest_tag; A.minActDist = V.minActDist; A.minTraceQuality = V.minTraceQuality;
    A.KRKi = t.d; A.Kt = t.d + 9 * V.n_hosts; A.flagged = reinterpret_cast<const unsigned char*>(t.d + 12 * V.n_hosts);
  }
  const int nmax = maxOf(nn);
  if (nmax > 0) {
    if (int r = b->slab.upload(st, L.bytes())) return r;
    HIPCHK(hipMemsetAsync(b->counts.d, 0, sizeof(int) * ACT_COUNTS * (size_t)W, st));
    const ActWin* D = b->slab.dev<const ActWin>(0);
    hipLaunchKernelGGL(k_act_classify_b, dim3((nmax + 255) / 256, W), dim3(256), 0, st, D, G);
    const int map_bytes = win[0].dm->map_bytes;
    if (lds) hipLaunchKernelGGL(k_act_ordered_walk_b<true>, dim3(W), dim3(ACT_THREADS), walkLds(true, map_bytes), st, D, G);
    else hipLaunchKernelGGL(k_act_ordered_walk_b<false>, dim3(W), dim3(ACT_THREADS), walkLds(false, 0), st, D, G);
    HIPCHK(hipGetLastError());
    if (int r = b->counts.download(st, 0, sizeof(int) * ACT_COUNTS * (size_t)W)) return r;
    if (int r = b->slab.wait(st)) return r;   // the one wait of the call
  }
  for (int w = 0; w < W; w++) {
    dmvio_hip_immature* m = win[w].imm;
    if (m->n > 0) {
      const int* hc = b->counts.host<int>(0) + (size_t)w * ACT_COUNTS;
      m->act_stats[0] = hc[ACTC_CLASSIFIED]; m->act_stats[1] = hc[ACTC_SURVIVORS]; m->act_stats[2] = hc[ACTC_ACCEPTED]; m->act_stats[3] = hc[ACTC_DELETED];
      m->n_selected = hc[ACTC_ACCEPTED];
    }
    m->have_selection = true;
    win[w].n_selected = m->n_selected; win[w].n_deleted = (int)m->act_stats[3];
  }
  return 0;
}

int dmvio_hip_immature_optimize_selected_batch(dmvio_hip_activation_batch* b, int W, dmvio_hip_activation_optimize* win, const double fxfycxcy[4]) {
  if (int r = dmvBatchHead(b, W, b ? b->max_windows : 0, win, "immature_optimize_selected_batch")) return r;
  if (W == 0) return 0;
  dmvio_hip_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  if (!fxfycxcy) return failmsg("immature_optimize_selected_batch: fxfycxcy is NULL");
  const int rep = dmvFirstRepeated(win, W, &dmvio_hip_activation_optimize::imm);
  for (int w = 0; w < W; w++) {
    const dmvio_hip_activation_optimize& V = win[w];
    if (!V.imm) return failmsg("immature_optimize_selected_batch: an immature handle is NULL");
    if (V.imm->ctx != c) return failmsg("immature_optimize_selected_batch: a handle belongs to another context");
    if (w == rep) return failmsg("immature_optimize_selected_batch: an immature handle appears twice");
    if (!V.imm->have_selection) return failmsg("immature_optimize_selected_batch: a handle has no selection (dmvio_hip_immature_select_for_activation_batch)");
    if (V.F < 2 || V.F > 8 || !V.frame_slots || !V.w2c7 || !V.aff2 || !V.exposure) return failmsg("immature_optimize_selected_batch: bad argument (F or a per-frame array)");
    if (V.imm->max_tag >= V.F) return failmsg("immature_optimize_selected_batch: a point's host_tag is not a keyframe index of its window (host_tag >= F)");
    for (int f = 0; f < V.F; f++) if (V.frame_slots[f] < 0 || V.frame_slots[f] >= c->n_slots) return failmsg("immature_optimize_selected_batch: frame slot out of range");
  }
  DmvCursor L; L.take<ActWin>(W);
  if (int r = batchBegin(b, L.bytes())) return r;
  hipStream_t st = c->stream;
  HIPCHK(hipStreamSynchronize(st));   // the handles' pinned tables are free to rewrite; nothing below waits until the end of the call
  std::vector<int> ns(W);
  for (int w = 0; w < W; w++) {
    dmvio_hip_activation_optimize& V = win[w];
    dmvio_hip_immature* m = V.imm;
    m->n_activated = 0; m->last_F = V.F; V.n_activated = 0;
    ns[w] = m->n_selected;
    if (ns[w] == 0) continue;
    if (int r = dmv_immature_optimize_launch_locked(m, V.F, V.frame_slots, V.w2c7, V.aff2, V.exposure, fxfycxcy, m->d_act_select, V.minObs, /*stream_idle=*/true)) return r;
  }
  const int smax = maxOf(ns);
  if (smax == 0) return 0;
  ActWin* R = b->slab.host<ActWin>(0);
  for (int w = 0; w < W; w++) { recordOf(R[w], b, w, win[w].imm, nullptr); R[w].F = win[w].F; }
  if (int r = b->slab.upload(st, L.bytes())) return r;
  HIPCHK(hipMemsetAsync(b->counts.d, 0, sizeof(int) * ACT_COUNTS * (size_t)W, st));
  hipLaunchKernelGGL(k_act_gather_b, dim3((smax + 255) / 256, W), dim3(256), 0, st, b->slab.dev<const ActWin>(0));
  HIPCHK(hipGetLastError());
  if (int r = b->counts.download(st, 0, sizeof(int) * ACT_COUNTS * (size_t)W)) return r;
  std::vector<std::vector<int>> rs8(W);
  for (int w = 0; w < W; w++) {
    dmvio_hip_activation_optimize& V = win[w];
    dmvio_hip_immature* m = V.imm;
    const size_t n = ns[w];
    if (!n) continue;
    if (V.result) HIPCHK(m->bounce.d2h(V.result, m->d_gather_i, sizeof(int) * n, st));
    if (V.idepth) HIPCHK(m->bounce.d2h(V.idepth, m->d_gather_f, sizeof(float) * n, st));
    if (V.res_state) { rs8[w].resize(8 * n); HIPCHK(m->bounce.d2h(rs8[w].data(), m->d_gather_i + 2 * n, sizeof(int) * 8 * n, st)); }
  }
  if (int r = b->slab.wait(st)) return r;   // the one wait for the results; the handles' deliveries below find the stream idle
  for (int w = 0; w < W; w++) {
    dmvio_hip_activation_optimize& V = win[w];
    dmvio_hip_immature* m = V.imm;
    if (!ns[w]) continue;
    HIPCHK(m->bounce.finish(st));
    if (V.res_state) for (int k = 0; k < ns[w]; k++) for (int t = 0; t < V.F; t++) V.res_state[(size_t)k * V.F + t] = rs8[w][8 * (size_t)k + t];
    m->n_activated = V.n_activated = b->counts.host<int>(0)[(size_t)w * ACT_COUNTS + ACTC_ACTIVATED];
  }
  return 0;
}

int dmvio_hip_immature_remove_marked_batch(dmvio_hip_activation_batch* b, int W, dmvio_hip_immature* const* imm, int* n_left) {
  if (int r = dmvBatchHead(b, W, b ? b->max_windows : 0, imm, "immature_remove_marked_batch")) return r;
  if (W == 0) return 0;
  dmvio_hip_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  const int rep = dmvFirstRepeated(reinterpret_cast<const void* const*>(imm), W);
  for (int w = 0; w < W; w++) {
    if (!imm[w]) return failmsg("immature_remove_marked_batch: an immature handle is NULL");
    if (imm[w]->ctx != c) return failmsg("immature_remove_marked_batch: a handle belongs to another context");
    if (w == rep) return failmsg("immature_remove_marked_batch: an immature handle appears twice");
    if (!imm[w]->have_selection) return failmsg("immature_remove_marked_batch: a handle has no marks (dmvio_hip_immature_select_for_activation_batch)");
  }
  DmvCursor L; L.take<ActWin>(W);
  if (int r = batchBegin(b, L.bytes())) return r;
  hipStream_t st = c->stream;
  ActWin* R = b->slab.host<ActWin>(0);
  std::vector<int> nn(W);
  for (int w = 0; w < W; w++) { recordOf(R[w], b, w, imm[w], nullptr); nn[w] = imm[w]->n; }
  const int nmax = maxOf(nn);
  if (nmax > 0) {
    if (int r = b->slab.upload(st, L.bytes())) return r;
    const ActWin* D = b->slab.dev<const ActWin>(0);
    hipLaunchKernelGGL(k_rm_plan_b, dim3(W), dim3(ACT_THREADS), 0, st, D);
    hipLaunchKernelGGL(k_rm_apply_b, dim3((nmax + 255) / 256, W), dim3(256), 0, st, D);
    HIPCHK(hipGetLastError());
    if (int r = b->counts.download(st, 0, sizeof(int) * ACT_COUNTS * (size_t)W)) return r;
    if (int r = b->slab.wait(st)) return r;   // the one wait of the call
  }
  for (int w = 0; w < W; w++) {
    dmvio_hip_immature* m = imm[w];
    if (m->n > 0) {
      const int* hc = b->counts.host<int>(0) + (size_t)w * ACT_COUNTS;
      const int n_tags = m->max_tag + 1;
      std::swap(m->P, m->P2);
      m->n = hc[ACTC_NEW_N];
      int mt = -1;
      for (int t = 0; t < n_tags; t++) if (hc[ACTC_TAGS + t] > 0) mt = t;
      m->max_tag = mt;
      m->P.n = m->n;
    }
    m->have_selection = false; m->n_selected = m->n_activated = 0;
    if (n_left) n_left[w] = m->n;
  }
  return 0;
}

}  // extern "C"
