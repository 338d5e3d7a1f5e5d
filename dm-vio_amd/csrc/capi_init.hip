// C ABI of the initializer hot function (include/dmvio_hip.h): CoarseInitializer::calcResAndGS, one window per call and W windows per call.
#include <vector>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <algorithm>
#include "../../include/dmvio_hip.h"
#include "internal.h"
#include "lie_dev.h"
#include "init_kernels.hpp"
#include "init_tail.hpp"
#include "init_handle.h"   // struct dmvio_hip_initializer, the evaluation's grid (initGrid) and what the resident unit (capi_init_resident.hip) borrows of this one

using namespace dmv;

// W windows per call.  The batch owns what a call needs besides the handles: a pinned slab and its device copy for the point sets of set_points_batch (the handles named there
// read their points from it until their next set_points: `tenants`), a pinned slab and its device copy for the records and idepth_new arrays of a calc call, the partials, and
// the sums and per-point results with the pinned slab they are downloaded into.  All grow on demand and are kept.
struct dmvio_hip_initializer_batch {
  dmvio_hip_ctx* ctx = nullptr;
  int max_windows = 0;
  DmvSlab pts;    // the point sets; busy() while the upload of the last set_points_batch may still read the pinned side
  std::vector<dmvio_hip_initializer*> tenants;
  DmvSlab up;     // [W InitWin | idepth_new of every window]
  DmvSlab part;   // the partials: device only
  DmvSlab dn;     // [W x IN_PART sums | results of the windows that asked for any | results of the others]
  DmvWork work;   // of the last calc call
};

template <class T>
static int nalloc(dmvio_hip_initializer* m, T** p, size_t n) {
  HIPCHK(hipMalloc((void**)p, sizeof(T) * std::max<size_t>(n, 1)));
  HIPCHK(hipMemset(*p, 0, sizeof(T) * std::max<size_t>(n, 1)));
  // hipMemset clears on the NULL stream without blocking the host, and the handle's stream is non-blocking: without this wait an upload enqueued next could
  // land before the clear does (seen with two processes sharing a GPU)
  HIPCHK(hipStreamSynchronize(nullptr));
  m->allocs.push_back(*p);
  return 0;
}
#define INIT_READY(m) do { if (!(m)) return failmsg("null initializer handle"); HIPCHK(hipSetDevice((m)->ctx->device)); } while (0)

// a slab of at least `need` bytes whose pinned side may be written; what it held is not kept (DmvSlab::reserve drains the stream before the old one is freed)
static int initReserve(DmvSlab& slab, size_t need, hipStream_t s) { if (int r = slab.reserve(need, std::max<size_t>(need + need / 2, 4096), s)) return r; return slab.begin(s); }
// the handle leaves its batch's slab.  keep: its point set goes back into its own d_in first (device to device, stream-ordered); otherwise it is about to be replaced.
static int initLeaveBatch(dmvio_hip_initializer* m, bool keep) {
  if (!m->owner) return 0;
  if (keep && m->n > 0) {
    const size_t P = padn(m->n);
    HIPCHK(hipMemcpyAsync(m->d_in, m->pts, sizeof(float) * 6 * P, hipMemcpyDeviceToDevice, m->ctx->stream));
    HIPCHK(hipMemcpyAsync(m->d_in + 7 * P, m->pts + 7 * P, m->n, hipMemcpyDeviceToDevice, m->ctx->stream));
  }
  std::vector<dmvio_hip_initializer*>& t = m->owner->tenants;
  t.erase(std::remove(t.begin(), t.end(), m), t.end());
  m->owner = nullptr;
  m->pts = m->d_in;
  return 0;
}

// [u | v | iR | outlierTH | energy(2) | (idepth_new) | isGood] of n points, the layout of d_in
static void initPackPoints(float* dst, int n, const float* u, const float* v, const float* iR, const unsigned char* isGood, const float* energy2, const float* outlierTH) {
  const size_t P = padn(n);
  memcpy(dst, u, sizeof(float) * n); memcpy(dst + P, v, sizeof(float) * n); memcpy(dst + 2 * P, iR, sizeof(float) * n);
  memcpy(dst + 3 * P, outlierTH, sizeof(float) * n); memcpy(dst + 4 * P, energy2, sizeof(float) * 2 * n);
  memcpy(dst + 7 * P, isGood, n);
}
// k_init_partial reads the first image at (u + dx, v + dy), dx, dy in [-2, 2], and one pixel right / below, without a test: CoarseInitializer::setFirst never
// places a point where that leaves the level, and a point set that does is refused (the staging slab still holds u, v and isGood of the last set_points).
// Returns the first offending point or -1.
static int initFirstPointOutside(const dmvio_hip_initializer* m, int lvl) {
  const dmvio_hip_ctx* c = m->ctx;
  const size_t P = padn(m->n);
  const float *u = m->h_in, *v = m->h_in + P;
  const unsigned char* good = reinterpret_cast<const unsigned char*>(m->h_in + 7 * P);
  const float umax = (float)(c->wl[lvl] - 3), vmax = (float)(c->hl[lvl] - 3);
  for (int i = 0; i < m->n; i++)
    if (good[i] && !(u[i] >= 2.0f && u[i] < umax && v[i] >= 2.0f && v[i] < vmax)) return i;
  return -1;
}
static std::string initOutsideMsg(const char* who, const dmvio_hip_initializer* m, int lvl, int i) {
  const dmvio_hip_ctx* c = m->ctx;
  char msg[224];
  snprintf(msg, sizeof(msg), "%sgood point %d at (%g, %g) outside [2, %d) x [2, %d) of level %d", who, i, (double)m->h_in[i], (double)m->h_in[padn(m->n) + i], c->wl[lvl] - 3,
           c->hl[lvl] - 3, lvl);
  return msg;
}
// the uniform inputs of the evaluation kernel (init_tail.hpp)
InitArgs initMakeArgs(const dmvio_hip_ctx* c, int lvl, const double Ki9[9], const float fxfycxcy_lvl[4], const Pose& T, const double aff_ab[2], int n, float alphaW,
                             float alphaK, float couplingWeight) {
  return initMakeArgsAt(c->wl[lvl], c->hl[lvl], Ki9, fxfycxcy_lvl, T, aff_ab, n, alphaW, alphaK, couplingWeight);
}
// where the kernel finds the n points of a handle and leaves their results (`res`: the layout of d_res)
static InitPts initMakePts(int n, float* in, const float* idepth_new, float* res) {
  const size_t PN = padn(n);
  InitPts P;
  P.n = n; P.u = in; P.v = in + PN; P.iR = in + 2 * PN; P.outlierTH = in + 3 * PN; P.energy = in + 4 * PN; P.idepth_new = idepth_new;
  P.isGood = reinterpret_cast<unsigned char*>(in + 7 * PN);
  P.energy_new = res; P.maxstep = res + 2 * PN; P.lastHessian_new = res + 3 * PN; P.JbBuffer_new = res + 4 * PN;
  P.isGood_new = reinterpret_cast<unsigned char*>(res + 14 * PN);
  return P;
}
// the per-point results from the downloaded slab (the layout of d_res) into the caller's arrays; each may be NULL
static void initDeliverPoints(const float* h_res, int n, float* energy_new2, unsigned char* isGood_new, float* maxstep, float* lastHessian_new, float* JbBuffer_new10) {
  const size_t PN = padn(n);
  if (energy_new2) memcpy(energy_new2, h_res, sizeof(float) * 2 * n);
  if (maxstep) memcpy(maxstep, h_res + 2 * PN, sizeof(float) * n);
  if (JbBuffer_new10) memcpy(JbBuffer_new10, h_res + 4 * PN, sizeof(float) * 10 * n);
  if (isGood_new) memcpy(isGood_new, h_res + 14 * PN, n);
  if (lastHessian_new) {
    // written for accepted points only, like the reference's member (CoarseInitializer.cpp:560): the kernel leaves the other entries of the slab as an earlier call,
    // laid out for another n, left them, so they are not the caller's to see
    const float* lh = h_res + 3 * PN;
    const unsigned char* acc = reinterpret_cast<const unsigned char*>(h_res + 14 * PN);
    for (int i = 0; i < n; i++) if (acc[i]) lastHessian_new[i] = lh[i];
  }
}
// the host tail of calcResAndGS, of the single and of the batched call (init_tail.hpp)
void initHostTail(const Pose& T, int n, float alphaW, float alphaK, double priorY, double priorX, const float* sums /* IN_PART */, float* H_out64, float* b_out8,
                         float* H_sc64, float* b_sc8, float res3[3]) {
  initTail(T, n, alphaW, alphaK, priorY, priorX, sums, H_out64, b_out8, H_sc64, b_sc8, res3, nullptr);
}

// the evaluation's two launches on the context's stream: the single call's grid, so the sums have the single call's bits wherever the points lie
int initLaunchEval(dmvio_hip_ctx* c, int lvl, int first_slot, int new_slot, const InitPts& P, const InitArgs& A, float* d_partials, float* d_out) {
  const int G = initGrid(P.n);
  hipLaunchKernelGGL(k_init_partial, dim3(G), dim3(256), 0, c->stream, c->frames.levelPtr(first_slot, lvl), c->frames.levelPtr(new_slot, lvl), P, A, d_partials);
  hipLaunchKernelGGL(k_init_final, dim3(1), dim3(128), 0, c->stream, d_partials, G, d_out);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" {

dmvio_hip_initializer* dmvio_hip_initializer_create(dmvio_hip_ctx* ctx, int capacity) {
  if (!ctx || capacity < 1) { failmsg("initializer_create: bad argument"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { failmsg("initializer_create: hipSetDevice failed"); return nullptr; }
  dmvio_hip_initializer* m = new dmvio_hip_initializer();
  m->ctx = ctx; m->capacity = capacity;
  const size_t c = padn(capacity);
  if (nalloc(m, &m->d_in, (IN_FLOATS + 1) * c) || nalloc(m, &m->d_res, (RES_FLOATS + 1) * c) || nalloc(m, &m->d_partials, (size_t)INIT_MAX_BLOCKS * IN_PART) ||
      nalloc(m, &m->d_out, IN_PART) || hipHostMalloc((void**)&m->h_out, sizeof(float) * IN_PART, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&m->h_in, sizeof(float) * (IN_FLOATS + 1) * c, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&m->h_res, sizeof(float) * (RES_FLOATS + 1) * c, hipHostMallocDefault) != hipSuccess) {
    for (void* p : m->allocs) hipFree(p);
    if (m->h_out) hipHostFree(m->h_out);
    if (m->h_in) hipHostFree(m->h_in);
    if (m->h_res) hipHostFree(m->h_res);
    delete m;
    return nullptr;
  }
  m->pts = m->d_in;
  return m;
}
void dmvio_hip_initializer_destroy(dmvio_hip_initializer* m) {
  if (!m) return;
  hipSetDevice(m->ctx->device);
  {
    std::lock_guard<std::mutex> lk(m->ctx->mu);
    initLeaveBatch(m, false);
  }
  hipStreamSynchronize(m->ctx->stream);
  dmvInitResidentRelease(m);
  for (void* p : m->allocs) hipFree(p);
  if (m->h_out) hipHostFree(m->h_out);
  if (m->h_in) hipHostFree(m->h_in);
  if (m->h_res) hipHostFree(m->h_res);
  delete m;
}

// the per-level point set (struct Pnt, CoarseInitializer.h:44-83): the fields calcResAndGS reads
int dmvio_hip_initializer_set_points(dmvio_hip_initializer* m, int n, const float* u, const float* v, const float* iR, const unsigned char* isGood,
                                     const float* energy2, const float* outlierTH) {
  INIT_READY(m);
  if (n < 0 || n > m->capacity || !u || !v || !iR || !isGood || !energy2 || !outlierTH) return failmsg("initializer_set_points: bad argument");
  std::lock_guard<std::mutex> lk(m->ctx->mu);   // (the handle may sit in a batch's slab: that list is the context's)
  hipStream_t s = m->ctx->stream;
  if (m->upload_pending) { HIPCHK(hipStreamSynchronize(s)); m->upload_pending = false; }   // the staging buffer is still being read by the previous upload
  if (int r = initLeaveBatch(m, false)) return r;
  const size_t P = padn(n);
  initPackPoints(m->h_in, n, u, v, iR, isGood, energy2, outlierTH);
  // [u | v | iR | outlierTH | energy] and, behind the gap idepth_new fills per evaluation, isGood: two copies, no wait — the evaluation's own synchronisation covers them
  HIPCHK(hipMemcpyAsync(m->d_in, m->h_in, sizeof(float) * 6 * P, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(m->d_in + 7 * P, m->h_in + 7 * P, n, hipMemcpyHostToDevice, s));
  m->upload_pending = true;
  m->n = n;
  return 0;
}

int dmvio_hip_initializer_calc_res_and_gs(dmvio_hip_initializer* m, int lvl, int first_slot, int new_slot, const double Ki9[9], const float fxfycxcy_lvl[4],
                                          const double refToNew7[7], const double aff_ab[2], const float* idepth_new, float alphaW, float alphaK,
                                          float couplingWeight, double priorY, double priorX, float* H_out64, float* b_out8, float* H_sc64, float* b_sc8,
                                          float res3[3], float* energy_new2, unsigned char* isGood_new, float* maxstep, float* lastHessian_new, float* JbBuffer_new10) {
  INIT_READY(m);
  dmvio_hip_ctx* c = m->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!Ki9 || !fxfycxcy_lvl || !refToNew7 || !aff_ab || !idepth_new || !H_out64 || !b_out8 || !H_sc64 || !b_sc8 || !res3) return failmsg("initializer_calc: null argument");
  if (lvl < 0 || lvl >= c->levels || first_slot < 0 || first_slot >= c->n_slots || new_slot < 0 || new_slot >= c->n_slots) return failmsg("initializer_calc: level / slot out of range");
  const int n = m->n;
  {
    const int i = initFirstPointOutside(m, lvl);
    if (i >= 0) return failmsg(initOutsideMsg("initializer_calc: ", m, lvl, i));
  }
  if (lvl == 0) { if (int r = dmv_ensure_row_major_locked(c, first_slot)) return r; if (int r = dmv_ensure_row_major_locked(c, new_slot)) return r; }
  hipStream_t s = c->stream;
  const Pose T = poseFrom7(refToNew7);
  const InitArgs A = initMakeArgs(c, lvl, Ki9, fxfycxcy_lvl, T, aff_ab, n, alphaW, alphaK, couplingWeight);
  const size_t PN = padn(n);
  memcpy(m->h_in + 6 * PN, idepth_new, sizeof(float) * n);
  HIPCHK(hipMemcpyAsync(m->pts + 6 * PN, m->h_in + 6 * PN, sizeof(float) * n, hipMemcpyHostToDevice, s));
  const InitPts P = initMakePts(n, m->pts, m->pts + 6 * PN, m->d_res);
  if (int r = initLaunchEval(c, lvl, first_slot, new_slot, P, A, m->d_partials, m->d_out)) return r;
  HIPCHK(hipMemcpyAsync(m->h_out, m->d_out, sizeof(float) * IN_PART, hipMemcpyDeviceToHost, s));
  const bool want = energy_new2 || isGood_new || maxstep || lastHessian_new || JbBuffer_new10;
  if (want) HIPCHK(hipMemcpyAsync(m->h_res, m->d_res, sizeof(float) * 14 * PN + n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  m->upload_pending = false;
  if (m->owner) m->owner->pts.settled();
  initDeliverPoints(m->h_res, n, energy_new2, isGood_new, maxstep, lastHessian_new, JbBuffer_new10);
  initHostTail(T, n, alphaW, alphaK, priorY, priorX, m->h_out, H_out64, b_out8, H_sc64, b_sc8, res3);
  return 0;
}

// ------------------------------------------------------------------------------------------------ W windows per call
dmvio_hip_initializer_batch* dmvio_hip_initializer_batch_create(dmvio_hip_ctx* ctx, int max_windows) {
  if (!ctx || max_windows < 1 || max_windows > 65535) { failmsg("initializer_batch_create: bad argument (max_windows in [1, 65535]: the window is a grid dimension)"); return nullptr; }
  dmvio_hip_initializer_batch* b = new dmvio_hip_initializer_batch();
  b->ctx = ctx; b->max_windows = max_windows;
  b->part.mirrors = 0;
  b->up.work = b->dn.work = &b->work;
  return b;
}
void dmvio_hip_initializer_batch_destroy(dmvio_hip_initializer_batch* b) {
  if (!b) return;
  hipSetDevice(b->ctx->device);
  {
    // the handles that still read their points from this batch's slab take them home first
    std::lock_guard<std::mutex> lk(b->ctx->mu);
    while (!b->tenants.empty()) initLeaveBatch(b->tenants.back(), true);
  }
  hipStreamSynchronize(b->ctx->stream);
  b->pts.release(); b->up.release(); b->part.release(); b->dn.release();
  delete b;
}

}  // extern "C"

// what both batched calls refuse of the call as a whole and of window i's handle; 0 or the failure
static int initBatchHead(const char* who, const dmvio_hip_initializer_batch* b, int W, const void* win) {
  char range[96];
  snprintf(range, sizeof(range), ": W = %d outside [0, %d]", W, b->max_windows);
  const char* const text[3] = {": null batch handle", range, ": null window array"};
  return dmvBatchHead(b, W, b->max_windows, win, who, text);
}
// rep: the first window that names an earlier window's handle (dmvFirstRepeated over the call's windows), or -1
template <class WIN>
static int initBatchCheckHandle(const char* who, const dmvio_hip_initializer_batch* b, const WIN* win, int i, int rep) {
  char msg[160];
  const dmvio_hip_initializer* m = win[i].ini;
  if (!m) { snprintf(msg, sizeof(msg), "%s: window %d: null initializer handle", who, i); return failmsg(msg); }
  if (m->ctx != b->ctx) { snprintf(msg, sizeof(msg), "%s: window %d: the initializer belongs to another context", who, i); return failmsg(msg); }
  if (i == rep) {
    int j = 0;
    while (win[j].ini != m) j++;
    snprintf(msg, sizeof(msg), "%s: window %d: the initializer of window %d named again", who, i, j); return failmsg(msg);
  }
  return 0;
}

extern "C" {

int dmvio_hip_initializer_set_points_batch(dmvio_hip_initializer_batch* b, int W, const dmvio_hip_initializer_points_window* win) {
  static const char* who = "initializer_set_points_batch";
  if (!b) return failmsg("initializer_set_points_batch: null batch handle");
  HIPCHK(hipSetDevice(b->ctx->device));
  dmvio_hip_ctx* c = b->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (int r = initBatchHead(who, b, W, win)) return r;
  const int rep = dmvFirstRepeated(win, W, &dmvio_hip_initializer_points_window::ini);
  for (int i = 0; i < W; i++) {
    if (int r = initBatchCheckHandle(who, b, win, i, rep)) return r;
    const dmvio_hip_initializer_points_window& w = win[i];
    if (w.n < 0 || w.n > w.ini->capacity || !w.u || !w.v || !w.iR || !w.isGood || !w.energy2 || !w.outlierTH) {
      char msg[160];
      snprintf(msg, sizeof(msg), "%s: window %d: bad argument (n = %d, capacity %d, or a null array)", who, i, w.n, w.ini->capacity);
      return failmsg(msg);
    }
  }
  if (W == 0) return 0;
  hipStream_t s = c->stream;
  // the pinned slabs written below may still be read by an earlier upload (the batch's, or a handle's own): the single call waits in the same case
  bool pending = b->pts.busy();
  for (int i = 0; i < W; i++) pending = pending || win[i].ini->upload_pending;
  if (pending) { HIPCHK(hipStreamSynchronize(s)); b->pts.settled(); for (int i = 0; i < W; i++) win[i].ini->upload_pending = false; }
  // the handles of this call move into this batch's slab, which is written from its start: those that live there and are not named again take their points home first
  for (int i = 0; i < W; i++) if (int r = initLeaveBatch(win[i].ini, false)) return r;
  while (!b->tenants.empty()) if (int r = initLeaveBatch(b->tenants.back(), true)) return r;
  DmvCursor L;   // per window the layout of d_in
  std::vector<size_t> off(W);
  for (int i = 0; i < W; i++) off[i] = L.take<float>((IN_FLOATS + 1) * padn(win[i].n));
  if (int r = initReserve(b->pts, L.bytes(), s)) return r;
  for (int i = 0; i < W; i++) {
    const dmvio_hip_initializer_points_window& w = win[i];
    dmvio_hip_initializer* m = w.ini;
    const auto at = b->pts.put<float>(off[i]);
    initPackPoints(at.h, w.n, w.u, w.v, w.iR, w.isGood, w.energy2, w.outlierTH);
    initPackPoints(m->h_in, w.n, w.u, w.v, w.iR, w.isGood, w.energy2, w.outlierTH);   // the handle's own staging copy: calc reads u, v and isGood there
    m->pts = at.d; m->owner = b; b->tenants.push_back(m);
    m->n = w.n;
    m->upload_pending = true;
  }
  // ONE copy, no wait: the evaluation's own synchronisation covers it
  if (L.bytes()) if (int r = b->pts.upload(s, L.bytes())) return r;
  return 0;
}

int dmvio_hip_initializer_calc_res_and_gs_batch(dmvio_hip_initializer_batch* b, int W, dmvio_hip_initializer_window* win) {
  static const char* who = "initializer_calc_batch";
  if (!b) return failmsg("initializer_calc_batch: null batch handle");
  HIPCHK(hipSetDevice(b->ctx->device));
  dmvio_hip_ctx* c = b->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (int r = initBatchHead(who, b, W, win)) return r;
  char msg[320];
  const int rep = dmvFirstRepeated(win, W, &dmvio_hip_initializer_window::ini);
  for (int i = 0; i < W; i++) {
    if (int r = initBatchCheckHandle(who, b, win, i, rep)) return r;
    const dmvio_hip_initializer_window& w = win[i];
    if (w.lvl < 0 || w.lvl >= c->levels || w.first_slot < 0 || w.first_slot >= c->n_slots || w.new_slot < 0 || w.new_slot >= c->n_slots) {
      snprintf(msg, sizeof(msg), "%s: window %d: level / slot out of range", who, i);
      return failmsg(msg);
    }
    if (w.ini->n > 0 && !w.idepth_new) { snprintf(msg, sizeof(msg), "%s: window %d: null idepth_new", who, i); return failmsg(msg); }
    const int p = initFirstPointOutside(w.ini, w.lvl);
    if (p >= 0) { snprintf(msg, sizeof(msg), "%s: window %d: ", who, i); return failmsg(initOutsideMsg(msg, w.ini, w.lvl, p)); }
  }
  b->work.clear();
  if (W == 0) return 0;
  // (not counted: the conversion of an 8x4-tiled level-0 slot, as in the single call)
  for (int i = 0; i < W; i++)
    if (win[i].lvl == 0) { if (int r = dmv_ensure_row_major_locked(c, win[i].first_slot)) return r; if (int r = dmv_ensure_row_major_locked(c, win[i].new_slot)) return r; }
  hipStream_t s = c->stream;
  // layout.  upload: [W records | idepth_new of window 0 | ...]; download: [W x IN_PART sums | results of the windows that asked for any | those of the others]
  DmvCursor up, dn;
  std::vector<size_t> id_off(W), res_off(W);
  std::vector<char> want(W);
  up.take<InitWin>(W); dn.take<float>((size_t)W * IN_PART);
  size_t parts = 0;
  int maxG = 1;
  for (int i = 0; i < W; i++) {
    const dmvio_hip_initializer_window& w = win[i];
    id_off[i] = up.take<float>(w.ini->n);
    want[i] = w.energy_new2 || w.isGood_new || w.maxstep || w.lastHessian_new || w.JbBuffer_new10;
    const int G = initGrid(w.ini->n);
    parts += (size_t)G; maxG = std::max(maxG, G);
  }
  size_t dn_wanted = 0;   // what comes back: the sums and the results somebody asked for
  for (int pass = 1; pass >= 0; pass--) {
    for (int i = 0; i < W; i++) if ((int)want[i] == pass) res_off[i] = dn.take<float>((RES_FLOATS + 1) * padn(win[i].ini->n));
    if (pass) dn_wanted = dn.bytes();
  }
  int held = initReserve(b->up, up.bytes(), s);
  if (held || (held = initReserve(b->part, sizeof(float) * parts * IN_PART, s)) || (held = initReserve(b->dn, dn.bytes(), s))) return held;
  InitWin* rec = b->up.host<InitWin>(0);
  std::vector<Pose> T(W);
  int part_off = 0;
  for (int i = 0; i < W; i++) {
    const dmvio_hip_initializer_window& w = win[i];
    dmvio_hip_initializer* m = w.ini;
    const int n = m->n;
    T[i] = poseFrom7(w.refToNew7);
    InitWin& R = rec[i];
    R.Iref = c->frames.levelPtr(w.first_slot, w.lvl); R.Inew = c->frames.levelPtr(w.new_slot, w.lvl);
    const auto idepth = b->up.put<float>(id_off[i]);
    R.P = initMakePts(n, m->pts, idepth.d, b->dn.dev<float>(res_off[i]));
    R.A = initMakeArgs(c, w.lvl, w.Ki9, w.fxfycxcy_lvl, T[i], w.aff_ab, n, w.alphaW, w.alphaK, w.couplingWeight);
    R.G = initGrid(n); R.part_off = part_off; R.sum_off = i * IN_PART;
    part_off += R.G;
    if (n > 0) memcpy(idepth.h, w.idepth_new, sizeof(float) * n);
  }
  if (int r = b->up.upload(s, up.bytes())) return r;
  const InitWin* d_rec = b->up.dev<const InitWin>(0);
  hipLaunchKernelGGL(k_init_partial_b, dim3(maxG, W), dim3(256), 0, s, d_rec, b->part.dev<float>(0)); b->work.launches++;
  hipLaunchKernelGGL(k_init_final_b, dim3(W), dim3(128), 0, s, d_rec, b->part.dev<const float>(0), b->dn.dev<float>(0)); b->work.launches++;
  HIPCHK(hipGetLastError());
  if (int r = b->dn.download(s, 0, dn_wanted)) return r;
  if (int r = b->up.wait(s)) return r;
  b->pts.settled();
  for (int i = 0; i < W; i++) {
    dmvio_hip_initializer_window& w = win[i];
    dmvio_hip_initializer* m = w.ini;
    m->upload_pending = false;
    if (m->owner) m->owner->pts.settled();
    if (want[i]) initDeliverPoints(b->dn.host<float>(res_off[i]), m->n, w.energy_new2, w.isGood_new, w.maxstep, w.lastHessian_new, w.JbBuffer_new10);
    initHostTail(T[i], m->n, w.alphaW, w.alphaK, w.priorY, w.priorX, b->dn.host<float>(0) + (size_t)i * IN_PART, w.H_out64, w.b_out8, w.H_sc64, w.b_sc8, w.res3);
  }
  return 0;
}

int dmvio_hip_initializer_batch_last_work(dmvio_hip_initializer_batch* b, int* launches, int* uploads, int* downloads, int* waits) {
  if (!b) return failmsg("initializer_batch_last_work: null batch handle");
  std::lock_guard<std::mutex> lk(b->ctx->mu);
  b->work.report(launches, uploads, downloads, waits);
  return 0;
}

}  // extern "C"
