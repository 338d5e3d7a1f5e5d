// C ABI of the immature-point path (include/dmvio_hip.h): ImmaturePoint construction and FullSystem::traceNewCoarse.
#include <vector>
#include <cmath>
#include <cstring>
#include "../../include/dmvio_hip.h"
#include "internal.h"
#include "lie_dev.h"
#include "immature_kernels.hpp"
#include "immature_handle.h"

using namespace dmv;

// ---- W windows per call: the slab of dmvio_hip_trace_batch (immature_handle.h) ----
static void traceBatchFree(dmvio_hip_trace_batch* b) {
  b->slab.release();
  if (b->h_counts) hipHostFree(b->h_counts);
  delete b;
}
// The body of both batched calls; the caller holds the context's mutex.  Every refusal comes before anything is enqueued or any handle touched.  counts: NULL, or 6 ints per
// window; then the histogram follows the trace and the stream is waited for once.
static int traceBatchLocked(dmvio_hip_trace_batch* b, int W, const dmvio_hip_trace_tables_window* win, int* counts, const char* what) {
  dmvio_hip_ctx* c = b->ctx;
  const std::string pre = std::string(what) + ": ";
  int nmax = 0;
  const int rep = dmvFirstRepeated(win, W, &dmvio_hip_trace_tables_window::imm);
  for (int k = 0; k < W; k++) {
    const dmvio_hip_trace_tables_window& V = win[k];
    if (!V.imm) return failmsg(pre + "an immature handle is NULL");
    if (V.imm->ctx != c) return failmsg(pre + "an immature handle belongs to another context");
    if (k == rep) return failmsg(pre + "an immature handle appears twice");
    if (V.new_slot < 0 || V.new_slot >= c->n_slots) return failmsg(pre + "frame slot out of range");
    if (V.n_hosts < 1 || V.n_hosts > IMM_MAX_HOSTS) return failmsg(pre + "n_hosts out of range (1..64)");
    if (!V.KRKi9 || !V.Kt3 || !V.aff2) return failmsg(pre + "a table is NULL");
    if (V.imm->n > 0 && V.imm->max_tag >= V.n_hosts) return failmsg(pre + "a point's host_tag has no table row (host_tag >= n_hosts)");
    nmax = std::max(nmax, V.imm->n);
  }
  for (int k = 0; k < W; k++) if (int r = dmv_ensure_row_major_locked(c, win[k].new_slot)) return r;
  if (counts) memset(counts, 0, sizeof(int) * 6 * (size_t)W);
  if (nmax == 0) return 0;   // every window is empty: nothing to launch
  if (int r = b->slab.begin(c->stream)) return r;   // this mirror's last upload, two calls ago: not the stream
  DmvCursor L;
  TraceWin* H = b->slab.host<TraceWin>(dmvRecords(L, sizeof(TraceWin), W));
  for (int k = 0; k < W; k++) {
    const dmvio_hip_trace_tables_window& V = win[k];
    dmvio_hip_immature* m = V.imm;
    const size_t nh = V.n_hosts;
    const auto t = b->slab.put<float>(dmvTraceTable(L, V.n_hosts));
    memcpy(t.h, V.KRKi9, sizeof(float) * 9 * nh); memcpy(t.h + 9 * nh, V.Kt3, sizeof(float) * 3 * nh); memcpy(t.h + 12 * nh, V.aff2, sizeof(float) * 2 * nh);
    m->P.n = m->n;
    TraceWin r{};
    r.I = c->frames.levelPtr(V.new_slot, 0); r.P = m->P; r.S = m->S;
    r.KRKi = t.d; r.Kt = t.d + 9 * nh; r.aff = t.d + 12 * nh;
    r.w = c->w; r.h = c->h;
    memcpy(&H[k], &r, sizeof(r));
  }
  if (int r = b->slab.upload(c->stream, L.bytes())) return r;
  const TraceWin* D = b->slab.dev<const TraceWin>(0);
  hipLaunchKernelGGL(k_immature_trace_b, dim3((nmax + 3) / 4, W), dim3(256), 0, c->stream, D);
  if (counts) hipLaunchKernelGGL(k_status_hist_b, dim3(W), dim3(1024), 0, c->stream, D, b->h_counts);
  HIPCHK(hipGetLastError());
  if (counts) {
    if (int r = b->slab.wait(c->stream)) return r;   // the call's one wait
    memcpy(counts, b->h_counts, sizeof(int) * 6 * (size_t)W);
  }
  return 0;
}

extern "C" {

dmvio_hip_immature* dmvio_hip_immature_create(dmvio_hip_ctx* ctx, int capacity) {
  if (!ctx || capacity < 1) { failmsg("immature_create: bad argument"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { failmsg("immature_create: hipSetDevice failed"); return nullptr; }
  dmvio_hip_immature* m = new dmvio_hip_immature();
  m->ctx = ctx; m->capacity = capacity;
  const size_t c = capacity;
  // two sets of per-point arrays: dmvio_hip_immature_remove_marked compacts from one into the other
  if (dmv_immature_alloc_pts(m, m->P) || dmv_immature_alloc_pts(m, m->P2) || ialloc(m, &m->d_tables, 14 * IMM_MAX_HOSTS) || ialloc(m, &m->d_uv_stage, 2 * c) ||
      ialloc(m, &m->d_opt_tables, 14 * 64) || ialloc(m, &m->d_result, c) || ialloc(m, &m->d_res_state, 8 * c) || ialloc(m, &m->d_idepth, c) || ialloc(m, &m->d_select, c) ||
      ialloc(m, &m->d_decision, c) || ialloc(m, &m->d_mark, c) || ialloc(m, &m->d_act_select, c) || ialloc(m, &m->d_order, c) || ialloc(m, &m->d_surv, c) || ialloc(m, &m->d_pidx, c) || ialloc(m, &m->d_frac, c) ||
      ialloc(m, &m->d_thr, c) || ialloc(m, &m->d_newidx, c) || ialloc(m, &m->d_holes, c) || ialloc(m, &m->d_act_counts, 8 + IMM_MAX_HOSTS) ||
      ialloc(m, &m->d_gather_i, (size_t)(2 + 8) * c) || ialloc(m, &m->d_gather_f, (size_t)(7 + 16) * c) ||
      hipHostMalloc((void**)&m->h_opt_tables, sizeof(float) * 14 * 64, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&m->h_tables, sizeof(float) * 14 * IMM_MAX_HOSTS, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&m->h_counts, sizeof(int) * (16 + IMM_MAX_HOSTS), hipHostMallocDefault) != hipSuccess) {
    for (void* p : m->allocs) hipFree(p);
    delete m;
    return nullptr;
  }
  return m;
}
void dmvio_hip_immature_destroy(dmvio_hip_immature* m) {
  if (!m) return;
  hipSetDevice(m->ctx->device);
  hipStreamSynchronize(m->ctx->stream);
  for (void* p : m->allocs) hipFree(p);
  if (m->h_tables) hipHostFree(m->h_tables);
  if (m->h_counts) hipHostFree(m->h_counts);
  if (m->h_opt_tables) hipHostFree(m->h_opt_tables);
  m->bounce.release();
  delete m;
}
int dmvio_hip_immature_clear(dmvio_hip_immature* m) { IMM_READY(m); m->n = 0; m->max_tag = -1; m->have_selection = false; m->n_selected = m->n_activated = 0; return 0; }
int dmvio_hip_immature_count(dmvio_hip_immature* m) { return m ? m->n : -1; }

int dmvio_hip_immature_add_points(dmvio_hip_immature* m, int host_tag, int host_slot, int n, const int* u, const int* v) {
  IMM_READY(m);
  dmvio_hip_ctx* c = m->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (n < 0 || !u || !v) return failmsg("immature_add_points: bad argument");
  if (m->n + n > m->capacity) return failmsg("immature_add_points: capacity exceeded");
  if (host_slot < 0 || host_slot >= c->n_slots || host_tag < 0 || host_tag >= IMM_MAX_HOSTS) return failmsg("immature_add_points: slot / tag out of range");
  if (int r = dmv_ensure_row_major_locked(c, host_slot)) return r;
  // the constructor reads the 2x2 cell of every pattern pixel: u +- 2 .. +1 must be inside the image (pixel selector margin, PixelSelector2.cpp)
  for (int i = 0; i < n; i++)
    if (u[i] < 2 || v[i] < 2 || u[i] + 3 >= c->w || v[i] + 3 >= c->h) return failmsg("immature_add_points: point closer than 3 px to the border");
  if (n == 0) return m->n;
  const int first = m->n;
  {
    // the integer pixel positions become the float arrays the kernels read, written straight into the pinned staging memory (no wait: the copies are ordered before the
    // constructor kernel on the stream, and the staging area is not reused before the next synchronisation)
    size_t off;   // ONE reservation for both arrays: a second one could drain and rewind the staging area under the first
    HIPCHK(m->bounce.reserve(sizeof(float) * 2 * (size_t)n, c->stream, &off));
    float* uf = reinterpret_cast<float*>(m->bounce.h + off); float* vf = uf + n;
    for (int i = 0; i < n; i++) { uf[i] = (float)u[i]; vf[i] = (float)v[i]; }
    HIPCHK(hipMemcpyAsync(m->P.u + first, uf, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(m->P.v + first, vf, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
  }
  m->P.n = first + n;
  hipLaunchKernelGGL(k_immature_init, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->frames.levelPtr(host_slot, 0), c->w, first, n, m->P, host_tag, m->S);
  HIPCHK(hipGetLastError());
  m->n = first + n;
  m->max_tag = std::max(m->max_tag, host_tag);
  return first;
}

// the loop of FullSystem::makeNewTraces (FullSystem.cpp:1653-1663) over the selector's device-resident list: the coordinates never visit the host, only their count does
int dmvio_hip_immature_add_selected(dmvio_hip_immature* m, int host_tag, int host_slot, dmvio_hip_pixel_selector* sel) {
  IMM_READY(m);
  dmvio_hip_ctx* c = m->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  dmvio_hip_ctx* sc = nullptr;
  const float *d_u = nullptr, *d_v = nullptr;
  const int n = dmv_selector_window_list(sel, &sc, &d_u, &d_v);
  if (n < 0) return n;
  if (sc != c) return failmsg("immature_add_selected: the selector belongs to another context");
  if (m->n + n > m->capacity) return failmsg("immature_add_selected: capacity exceeded");
  if (host_slot < 0 || host_slot >= c->n_slots || host_tag < 0 || host_tag >= IMM_MAX_HOSTS) return failmsg("immature_add_selected: slot / tag out of range");
  if (int r = dmv_ensure_row_major_locked(c, host_slot)) return r;
  if (n == 0) return m->n;
  const int first = m->n;
  // the window (3 <= x < w-4, 3 <= y < h-4) lies inside the margin the constructor needs (dmvio_hip_immature_add_points)
  HIPCHK(hipMemcpyAsync(m->P.u + first, d_u, sizeof(float) * n, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(m->P.v + first, d_v, sizeof(float) * n, hipMemcpyDeviceToDevice, c->stream));
  m->P.n = first + n;
  hipLaunchKernelGGL(k_immature_init, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->frames.levelPtr(host_slot, 0), c->w, first, n, m->P, host_tag, m->S);
  hipLaunchKernelGGL(k_immature_types_from_map, dim3((n + 255) / 256), dim3(256), 0, c->stream, dmv_selector_map(sel), c->w, first, n, m->P);
  HIPCHK(hipGetLastError());
  m->n = first + n;
  m->max_tag = std::max(m->max_tag, host_tag);
  return first;
}

// the same loop for W windows: one record upload, one launch sequence (coordinate copy + constructor, then the types from the map); like the single call it does not wait
int dmvio_hip_immature_add_selected_batch(dmvio_hip_pixel_selector_batch* batch, int W, dmvio_hip_new_traces_window* win) {
  dmvio_hip_ctx* c = nullptr;
  int max_windows = 0;
  char* d_records = nullptr;
  if (int r = dmv_selector_batch_traces(batch, sizeof(NewTracesWin), &c, &max_windows, &d_records)) return r;
  if (int r = dmvBatchHead(batch, W, max_windows, win, "immature_add_selected_batch")) return r;
  if (W == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  // every refusal before anything is enqueued or any handle touched
  std::vector<int> nn(W);
  std::vector<const float*> du(W), dv(W);
  const int rep = dmvFirstRepeated(win, W, &dmvio_hip_new_traces_window::imm);
  for (int k = 0; k < W; k++) {
    const dmvio_hip_new_traces_window& V = win[k];
    if (!V.imm) return failmsg("immature_add_selected_batch: an immature handle is NULL");
    if (!V.sel) return failmsg("immature_add_selected_batch: a selector handle is NULL");
    if (V.imm->ctx != c) return failmsg("immature_add_selected_batch: an immature handle belongs to another context");
    if (k == rep) return failmsg("immature_add_selected_batch: an immature handle appears twice");
    dmvio_hip_ctx* sc = nullptr;
    nn[k] = dmv_selector_window_list(V.sel, &sc, &du[k], &dv[k]);
    if (nn[k] < 0) return nn[k];
    if (sc != c) return failmsg("immature_add_selected_batch: a selector belongs to another context");
    if (V.imm->n + nn[k] > V.imm->capacity) return failmsg("immature_add_selected_batch: capacity exceeded");
    if (V.host_slot < 0 || V.host_slot >= c->n_slots || V.host_tag < 0 || V.host_tag >= IMM_MAX_HOSTS) return failmsg("immature_add_selected_batch: slot / tag out of range");
  }
  for (int k = 0; k < W; k++) if (int r = dmv_ensure_row_major_locked(c, win[k].host_slot)) return r;
  int nmax = 0;
  for (int k = 0; k < W; k++) nmax = std::max(nmax, nn[k]);
  if (nmax > 0) {
    // the records are staged in the context's pinned memory, which stays intact until the next wait on the stream
    size_t off;
    HIPCHK(c->bounce.reserve(sizeof(NewTracesWin) * (size_t)W, c->stream, &off));
    NewTracesWin* R = reinterpret_cast<NewTracesWin*>(c->bounce.h + off);
    for (int k = 0; k < W; k++) {
      const dmvio_hip_new_traces_window& V = win[k];
      NewTracesWin r{};
      r.I = c->frames.levelPtr(V.host_slot, 0); r.wu = du[k]; r.wv = dv[k]; r.map = dmv_selector_map(V.sel);
      r.P = V.imm->P; r.P.n = V.imm->n + nn[k];
      r.S = V.imm->S;
      r.w = c->w; r.first = V.imm->n; r.n = nn[k]; r.host_tag = V.host_tag;
      memcpy(&R[k], &r, sizeof(r));
    }
    HIPCHK(hipMemcpyAsync(d_records, R, sizeof(NewTracesWin) * (size_t)W, hipMemcpyHostToDevice, c->stream));
    const NewTracesWin* D = reinterpret_cast<const NewTracesWin*>(d_records);
    // the window (3 <= x < w-4, 3 <= y < h-4) lies inside the margin the constructor needs (dmvio_hip_immature_add_points)
    hipLaunchKernelGGL(k_immature_init_b, dim3((nmax + 255) / 256, W), dim3(256), 0, c->stream, D);
    hipLaunchKernelGGL(k_immature_types_from_map_b, dim3((nmax + 255) / 256, W), dim3(256), 0, c->stream, D);
    HIPCHK(hipGetLastError());
  }
  for (int k = 0; k < W; k++) {
    dmvio_hip_immature* m = win[k].imm;
    win[k].first = m->n;
    if (nn[k] == 0) continue;   // as the single call: nothing added, nothing changed
    m->P.n = m->n + nn[k];
    m->n += nn[k];
    m->max_tag = std::max(m->max_tag, win[k].host_tag);
  }
  return 0;
}

int dmvio_hip_immature_get_static(dmvio_hip_immature* m, float* u, float* v, int* host_tag, float* color8, float* weights8, float* gradH4, float* energyTH) {
  IMM_READY(m);
  hipStream_t s = m->ctx->stream;
  const size_t n = m->n;
  if (u) HIPCHK(m->bounce.d2h(u, m->P.u, sizeof(float) * n, s));
  if (v) HIPCHK(m->bounce.d2h(v, m->P.v, sizeof(float) * n, s));
  if (host_tag) HIPCHK(m->bounce.d2h(host_tag, m->P.host, sizeof(int) * n, s));
  if (color8) HIPCHK(m->bounce.d2h(color8, m->P.color, sizeof(float) * 8 * n, s));
  if (weights8) HIPCHK(m->bounce.d2h(weights8, m->P.weights, sizeof(float) * 8 * n, s));
  if (gradH4) HIPCHK(m->bounce.d2h(gradH4, m->P.gradH, sizeof(float) * 4 * n, s));
  if (energyTH) HIPCHK(m->bounce.d2h(energyTH, m->P.energyTH, sizeof(float) * n, s));
  HIPCHK(m->bounce.finish(s));
  return 0;
}
int dmvio_hip_immature_get_state(dmvio_hip_immature* m, float* idepth_min, float* idepth_max, float* quality, float* lastTraceUV2, float* lastTracePixelInterval,
                                 int* lastTraceStatus) {
  IMM_READY(m);
  hipStream_t s = m->ctx->stream;
  const size_t n = m->n;
  if (idepth_min) HIPCHK(m->bounce.d2h(idepth_min, m->P.idepth_min, sizeof(float) * n, s));
  if (idepth_max) HIPCHK(m->bounce.d2h(idepth_max, m->P.idepth_max, sizeof(float) * n, s));
  if (quality) HIPCHK(m->bounce.d2h(quality, m->P.quality, sizeof(float) * n, s));
  if (lastTraceUV2) HIPCHK(m->bounce.d2h(lastTraceUV2, m->P.lastTraceUV, sizeof(float) * 2 * n, s));
  if (lastTracePixelInterval) HIPCHK(m->bounce.d2h(lastTracePixelInterval, m->P.lastTracePixelInterval, sizeof(float) * n, s));
  if (lastTraceStatus) HIPCHK(m->bounce.d2h(lastTraceStatus, m->P.lastTraceStatus, sizeof(int) * n, s));
  HIPCHK(m->bounce.finish(s));
  return 0;
}
int dmvio_hip_immature_set_state(dmvio_hip_immature* m, const float* idepth_min, const float* idepth_max, const float* quality, const int* lastTraceStatus) {
  IMM_READY(m);
  hipStream_t s = m->ctx->stream;
  const size_t n = m->n;
  if (idepth_min) HIPCHK(m->bounce.h2d(m->P.idepth_min, idepth_min, sizeof(float) * n, s));
  if (idepth_max) HIPCHK(m->bounce.h2d(m->P.idepth_max, idepth_max, sizeof(float) * n, s));
  if (quality) HIPCHK(m->bounce.h2d(m->P.quality, quality, sizeof(float) * n, s));
  if (lastTraceStatus) HIPCHK(m->bounce.h2d(m->P.lastTraceStatus, lastTraceStatus, sizeof(int) * n, s));
  HIPCHK(m->bounce.finish(s));
  return 0;
}

// traceOn of every point against the frame in new_slot; per-host tables indexed by the points' host_tag
int dmvio_hip_immature_trace(dmvio_hip_immature* m, int new_slot, int n_hosts, const float* KRKi9, const float* Kt3, const float* aff2) {
  IMM_READY(m);
  dmvio_hip_ctx* c = m->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!KRKi9 || !Kt3 || !aff2 || n_hosts < 1 || n_hosts > IMM_MAX_HOSTS) return failmsg("immature_trace: bad argument");
  if (new_slot < 0 || new_slot >= c->n_slots) return failmsg("immature_trace: frame slot out of range");
  if (int r = dmv_ensure_row_major_locked(c, new_slot)) return r;
  if (m->n == 0) return 0;
  if (m->max_tag >= n_hosts) return failmsg("immature_trace: a point's host_tag has no table row (host_tag >= n_hosts)");
  m->P.n = m->n;
  if (n_hosts <= IMM_ARG_HOSTS) {
    TraceTablesArg T;
    memset(&T, 0, sizeof(T));
    memcpy(T.KRKi, KRKi9, sizeof(float) * 9 * n_hosts);
    memcpy(T.Kt, Kt3, sizeof(float) * 3 * n_hosts);
    memcpy(T.aff, aff2, sizeof(float) * 2 * n_hosts);
    hipLaunchKernelGGL(k_immature_trace<TraceTablesArg>, dim3((m->n + 3) / 4), dim3(256), 0, c->stream, c->frames.levelPtr(new_slot, 0), c->w, c->h, m->P, T, m->S);
  } else {
    HIPCHK(hipStreamSynchronize(c->stream));   // the pinned tables of a previous call may still be in flight
    float* t = m->h_tables;
    memcpy(t, KRKi9, sizeof(float) * 9 * n_hosts);
    memcpy(t + 9 * IMM_MAX_HOSTS, Kt3, sizeof(float) * 3 * n_hosts);
    memcpy(t + 12 * IMM_MAX_HOSTS, aff2, sizeof(float) * 2 * n_hosts);
    HIPCHK(hipMemcpyAsync(m->d_tables, t, sizeof(float) * 14 * IMM_MAX_HOSTS, hipMemcpyHostToDevice, c->stream));
    TraceTables T;
    T.KRKi = m->d_tables; T.Kt = m->d_tables + 9 * IMM_MAX_HOSTS; T.aff = m->d_tables + 12 * IMM_MAX_HOSTS;
    hipLaunchKernelGGL(k_immature_trace<TraceTables>, dim3((m->n + 3) / 4), dim3(256), 0, c->stream, c->frames.levelPtr(new_slot, 0), c->w, c->h, m->P, T, m->S);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// FullSystem::traceNewCoarse (FullSystem.cpp:541-584): per-host KRKi / Kt / affine tables from the poses, traceOn of every immature point,
// status histogram counts6 = {good, oob, outlier, skipped, badcondition, uninitialized}
int dmvio_hip_trace_new_coarse(dmvio_hip_immature* m, int new_slot, const double new_w2c7[7], const double new_aff[2], float new_exposure, int n_hosts,
                               const double* host_c2w7, const double* host_aff2, const float* host_exposure, const double fxfycxcy[4], int counts6[6]) {
  IMM_READY(m);
  if (!new_w2c7 || !new_aff || !host_c2w7 || !host_aff2 || !host_exposure || !fxfycxcy || n_hosts < 1 || n_hosts > IMM_MAX_HOSTS) return failmsg("trace_new_coarse: bad argument");
  std::vector<float> KRKi(9 * (size_t)n_hosts), Kt(3 * (size_t)n_hosts), aff(2 * (size_t)n_hosts);
  const float K[9] = {(float)fxfycxcy[0], 0, (float)fxfycxcy[2], 0, (float)fxfycxcy[1], (float)fxfycxcy[3], 0, 0, 1};
  dmv_host_tables(K, fxfycxcy, new_w2c7, n_hosts, host_c2w7, KRKi.data(), Kt.data());
  for (int hI = 0; hI < n_hosts; hI++) {
    double ab[2];
    affFromTo(host_exposure[hI], new_exposure, host_aff2[2 * hI], host_aff2[2 * hI + 1], new_aff[0], new_aff[1], ab);
    aff[2 * hI] = (float)ab[0]; aff[2 * hI + 1] = (float)ab[1];
  }
  if (int r = dmvio_hip_immature_trace(m, new_slot, n_hosts, KRKi.data(), Kt.data(), aff.data())) return r;
  if (counts6) {
    for (int k = 0; k < 6; k++) counts6[k] = 0;
    if (m->n > 0) {
      dmvio_hip_ctx* c = m->ctx;
      std::lock_guard<std::mutex> lk(c->mu);
      hipLaunchKernelGGL(k_status_hist, dim3(1), dim3(1024), 0, c->stream, (const int*)m->P.lastTraceStatus, m->n, m->h_counts);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(c->stream));
      for (int k = 0; k < 6; k++) counts6[k] = m->h_counts[k];
    }
  }
  return 0;
}

// ---- W windows per call ----
dmvio_hip_trace_batch* dmvio_hip_trace_batch_create(dmvio_hip_ctx* ctx, int max_windows) {
  if (!ctx) { failmsg("trace_batch_create: null context"); return nullptr; }
  if (max_windows < 1 || max_windows > 65535) { failmsg("trace_batch_create: max_windows out of range (1..65535)"); return nullptr; }
  HIPCHKP(hipSetDevice(ctx->device));
  dmvio_hip_trace_batch* b = new dmvio_hip_trace_batch();
  b->ctx = ctx; b->max_windows = max_windows;
  if (b->slab.create(dmvTraceSlabBytes(sizeof(TraceWin), max_windows, IMM_MAX_HOSTS), 2, true) ||
      hipHostMalloc((void**)&b->h_counts, sizeof(int) * 6 * (size_t)max_windows, hipHostMallocDefault) != hipSuccess) {
    failmsg("trace_batch_create: allocation failed");
    traceBatchFree(b);
    return nullptr;
  }
  return b;
}
void dmvio_hip_trace_batch_destroy(dmvio_hip_trace_batch* b) {
  if (!b) return;
  hipSetDevice(b->ctx->device);
  hipStreamSynchronize(b->ctx->stream);
  traceBatchFree(b);
}

// traceOn of every point of every window: as dmvio_hip_immature_trace it does not wait
int dmvio_hip_immature_trace_batch(dmvio_hip_trace_batch* b, int W, const dmvio_hip_trace_tables_window* win) {
  if (int r = dmvBatchHead(b, W, b ? b->max_windows : 0, win, "immature_trace_batch")) return r;
  if (W == 0) return 0;
  HIPCHK(hipSetDevice(b->ctx->device));
  std::lock_guard<std::mutex> lk(b->ctx->mu);
  return traceBatchLocked(b, W, win, nullptr, "immature_trace_batch");
}

// FullSystem::traceNewCoarse (FullSystem.cpp:541-584) for every window: the tables of each window from its poses by the single call's host functions, one trace launch, and
// with want_counts one histogram launch and the call's only wait
int dmvio_hip_trace_new_coarse_batch(dmvio_hip_trace_batch* b, int W, dmvio_hip_trace_window* win, const double fxfycxcy[4], int want_counts) {
  if (int r = dmvBatchHead(b, W, b ? b->max_windows : 0, win, "trace_new_coarse_batch")) return r;
  if (!fxfycxcy) return failmsg("trace_new_coarse_batch: fxfycxcy is NULL");
  if (W == 0) return 0;
  size_t rows = 0;
  for (int k = 0; k < W; k++) {
    const dmvio_hip_trace_window& V = win[k];
    if (V.n_hosts < 1 || V.n_hosts > IMM_MAX_HOSTS) return failmsg("trace_new_coarse_batch: n_hosts out of range (1..64)");
    if (!V.host_c2w7 || !V.host_aff2 || !V.host_exposure) return failmsg("trace_new_coarse_batch: a pose, affine or exposure array is NULL");
    rows += V.n_hosts;
  }
  std::vector<float> tab(14 * rows);
  std::vector<dmvio_hip_trace_tables_window> tw(W);
  const float K[9] = {(float)fxfycxcy[0], 0, (float)fxfycxcy[2], 0, (float)fxfycxcy[1], (float)fxfycxcy[3], 0, 0, 1};
  float* t = tab.data();
  for (int k = 0; k < W; k++) {
    const dmvio_hip_trace_window& V = win[k];
    float *KRKi = t, *Kt = t + 9 * V.n_hosts, *aff = t + 12 * V.n_hosts;
    t += 14 * V.n_hosts;
    dmv_host_tables(K, fxfycxcy, V.new_w2c7, V.n_hosts, V.host_c2w7, KRKi, Kt);
    for (int hI = 0; hI < V.n_hosts; hI++) {
      double ab[2];
      affFromTo(V.host_exposure[hI], V.new_exposure, V.host_aff2[2 * hI], V.host_aff2[2 * hI + 1], V.new_aff[0], V.new_aff[1], ab);
      aff[2 * hI] = (float)ab[0]; aff[2 * hI + 1] = (float)ab[1];
    }
    tw[k].imm = V.imm; tw[k].new_slot = V.new_slot; tw[k].n_hosts = V.n_hosts; tw[k].KRKi9 = KRKi; tw[k].Kt3 = Kt; tw[k].aff2 = aff;
  }
  HIPCHK(hipSetDevice(b->ctx->device));
  std::lock_guard<std::mutex> lk(b->ctx->mu);
  if (!want_counts) return traceBatchLocked(b, W, tw.data(), nullptr, "trace_new_coarse_batch");
  std::vector<int> counts(6 * (size_t)W);
  if (int r = traceBatchLocked(b, W, tw.data(), counts.data(), "trace_new_coarse_batch")) return r;
  for (int k = 0; k < W; k++) memcpy(win[k].counts6, &counts[6 * (size_t)k], sizeof(int) * 6);
  return 0;
}

// FullSystem::optimizeImmaturePoint for the selected points (FullSystemOptPoint.cpp:51-205; caller: activatePointsMT_Reductor,
// FullSystem.cpp:587-602).  The pair tables PRE_RTll / PRE_tTll / PRE_aff_mode are FrameFramePrecalc::set (HessianBlocks.cpp:193-223).
int dmvio_hip_immature_optimize(dmvio_hip_immature* m, int F, const int* frame_slots, const double* w2c7, const double* aff2, const float* exposure,
                                const double fxfycxcy[4], const unsigned char* select, int minObs, int* result, float* idepth, int* res_state) {
  IMM_READY(m);
  dmvio_hip_ctx* c = m->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!result || !idepth) return failmsg("immature_optimize: bad argument");
  if (m->n == 0) return 0;
  if (select) HIPCHK(m->bounce.h2d(m->d_select, select, m->n, c->stream));
  if (int r = dmv_immature_optimize_launch_locked(m, F, frame_slots, w2c7, aff2, exposure, fxfycxcy, select ? m->d_select : nullptr, minObs)) return r;
  HIPCHK(m->bounce.d2h(result, m->d_result, sizeof(int) * m->n, c->stream));
  HIPCHK(m->bounce.d2h(idepth, m->d_idepth, sizeof(float) * m->n, c->stream));
  if (res_state) HIPCHK(m->bounce.d2h(res_state, m->d_res_state, sizeof(int) * (size_t)m->n * F, c->stream));
  HIPCHK(m->bounce.finish(c->stream));
  return 0;
}

}  // extern "C"

int dmv_immature_optimize_launch_locked(dmvio_hip_immature* m, int F, const int* frame_slots, const double* w2c7, const double* aff2, const float* exposure,
                                        const double fxfycxcy[4], const unsigned char* d_mask, int minObs, bool stream_idle) {
  dmvio_hip_ctx* c = m->ctx;
  if (F < 2 || F > 8 || !frame_slots || !w2c7 || !aff2 || !exposure || !fxfycxcy) return failmsg("immature_optimize: bad argument");
  if (m->n == 0) return 0;
  if (m->max_tag >= F) return failmsg("immature_optimize: a point's host_tag is not a keyframe index of this window (host_tag >= F)");
  if (!stream_idle) HIPCHK(hipStreamSynchronize(c->stream));
  float* tb = m->h_opt_tables;
  float *R = tb, *t = tb + 9 * 64, *aff = tb + 12 * 64;
  OptTables T;
  T.F = F;
  for (int f = 0; f < 8; f++) T.slot[f] = 0;
  for (int f = 0; f < F; f++) {
    if (frame_slots[f] < 0 || frame_slots[f] >= c->n_slots) return failmsg("immature_optimize: frame slot out of range");
    if (int r = dmv_ensure_row_major_locked(c, frame_slots[f])) return r;
    T.slot[f] = frame_slots[f];
  }
  for (int hI = 0; hI < F; hI++) {
    const Pose c2w = poseInv(poseFrom7(w2c7 + 7 * hI));
    for (int tI = 0; tI < F; tI++) {
      const Pose l = poseMul(poseFrom7(w2c7 + 7 * tI), c2w);
      double Rd[9];
      quatToR(l.q, Rd);
      const int o = hI * F + tI;
      for (int i = 0; i < 9; i++) R[9 * o + i] = (float)Rd[i];
      for (int i = 0; i < 3; i++) t[3 * o + i] = (float)l.t[i];
      double ab[2];
      affFromTo(exposure[hI], exposure[tI], aff2[2 * hI], aff2[2 * hI + 1], aff2[2 * tI], aff2[2 * tI + 1], ab);
      aff[2 * o] = (float)ab[0]; aff[2 * o + 1] = (float)ab[1];
    }
  }
  HIPCHK(hipMemcpyAsync(m->d_opt_tables, tb, sizeof(float) * 14 * 64, hipMemcpyHostToDevice, c->stream));
  T.R = m->d_opt_tables; T.t = m->d_opt_tables + 9 * 64; T.aff = m->d_opt_tables + 12 * 64;
  T.fxl = (float)fxfycxcy[0]; T.fyl = (float)fxfycxcy[1]; T.cxl = (float)fxfycxcy[2]; T.cyl = (float)fxfycxcy[3];
  T.fxli = 1.0f / T.fxl; T.fyli = 1.0f / T.fyl;   // CalibHessian::setValueScaled (HessianBlocks.h:373-387)
  m->P.n = m->n;
  hipLaunchKernelGGL(k_immature_optimize, dim3((m->n + 3) / 4), dim3(256), 0, c->stream, c->frames.built_and_waited(), c->w, c->h, m->P, T, d_mask, minObs,
                     100.0f /* setting_minIdepthH_act */, 3 /* setting_GNItsOnPointActivation */, m->S.huberTH, m->d_result, m->d_idepth, m->d_res_state);
  HIPCHK(hipGetLastError());
  return 0;
}

void dmv_host_tables(const float K[9], const double fxfycxcy[4], const double new_w2c7[7], int n_hosts, const double* host_c2w7, float* KRKi, float* Kt) {
  const float fx = (float)fxfycxcy[0], fy = (float)fxfycxcy[1], cx = (float)fxfycxcy[2], cy = (float)fxfycxcy[3];
  // K0.inverse(): Eigen's 3x3 cofactor inverse
  const float a = fx, e = fy, cc = cx, ff = cy;
  const float det = a * (e * 1.0f - ff * 0.0f), invdet = 1.0f / det;
  const float Ki[9] = {(e * 1.0f - ff * 0.0f) * invdet, (cc * 0.0f - 0.0f * 1.0f) * invdet, (0.0f * ff - cc * e) * invdet,
                       (ff * 0.0f - 0.0f * 1.0f) * invdet, (a * 1.0f - cc * 0.0f) * invdet, (cc * 0.0f - a * ff) * invdet,
                       (0.0f * 0.0f - e * 0.0f) * invdet, (0.0f * 0.0f - a * 0.0f) * invdet, (a * e - 0.0f * 0.0f) * invdet};
  const Pose Tn = poseFrom7(new_w2c7);
  for (int hI = 0; hI < n_hosts; hI++) {
    const Pose T = poseMul(Tn, poseFrom7(host_c2w7 + 7 * hI));
    double Rd[9];
    quatToR(T.q, Rd);
    float R[9], t[3], KR[9];
    for (int i = 0; i < 9; i++) R[i] = (float)Rd[i];
    for (int i = 0; i < 3; i++) t[i] = (float)T.t[i];
    for (int r = 0; r < 3; r++) for (int q = 0; q < 3; q++) KR[r * 3 + q] = K[r * 3 + 0] * R[q] + K[r * 3 + 1] * R[3 + q] + K[r * 3 + 2] * R[6 + q];
    for (int r = 0; r < 3; r++) for (int q = 0; q < 3; q++) KRKi[9 * hI + r * 3 + q] = KR[r * 3 + 0] * Ki[q] + KR[r * 3 + 1] * Ki[3 + q] + KR[r * 3 + 2] * Ki[6 + q];
    for (int r = 0; r < 3; r++) Kt[3 * hI + r] = K[r * 3 + 0] * t[0] + K[r * 3 + 1] * t[1] + K[r * 3 + 2] * t[2];
  }
}
