// C ABI of point activation (include/dmvio_hip.h): CoarseDistanceMap, the candidate loop and the compaction of FullSystem::activatePointsMT.
#include <vector>
#include <cmath>
#include <cstring>
#include <algorithm>
#include "../../include/dmvio_hip.h"
#include "internal.h"
#include "immature_handle.h"
#include "activate_kernels.hpp"

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
