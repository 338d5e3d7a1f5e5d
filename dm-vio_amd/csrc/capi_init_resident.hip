// C ABI of the resident initializer (include/dmvio_hip_init_resident.h): the point set of a level and both JbBuffers in device memory, and the per-point passes of
// CoarseInitializer::trackFrame (src/dso/FullSystem/CoarseInitializer.cpp) on them.  The evaluation is capi_init.hip's (initLaunchEval): the same kernels on the same grid.
#include <vector>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <algorithm>
#include "../../include/dmvio_hip_init_resident.h"
#include "init_handle.h"
#include "init_resident_state.h"
#include "init_resident_host.hpp"
#include "init_resident_kernels.hpp"

using namespace dmv;

void dmvInitResidentRelease(dmvio_hip_initializer* m) {
  if (!m->resident) return;
  m->resident->st.release(); m->resident->io.release();
  delete m->resident;
  m->resident = nullptr;
}

// the head of every resident_ call: the handle, its device, then — under the lock — its resident state.  Counted work restarts behind a calc or get_state.
#define RES_HEAD(m, who)                                                                                          \
  if (!(m)) return failmsg(who ": null initializer handle");                                                      \
  HIPCHK(hipSetDevice((m)->ctx->device));                                                                         \
  dmvio_hip_ctx* c = (m)->ctx;                                                                                    \
  std::lock_guard<std::mutex> lk(c->mu);                                                                          \
  if (!(m)->resident || !(m)->resident->live) return failmsg(who ": the handle has no resident point set (dmvio_hip_initializer_set_resident)"); \
  DmvInitResident* R = (m)->resident;                                                                             \
  hipStream_t s = c->stream;                                                                                      \
  (void)s
static void resOpen(DmvInitResident* R) { if (R->work_closed) { R->work.clear(); R->work_closed = false; } }
static inline dim3 resGrid(int n) { return dim3((unsigned)((n + 255) / 256)); }

static int resAllowLds(DmvInitResident* R, int device) {
  if (R->lds_limit) return 0;
  int lim = 0;
  HIPCHK(hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  if (lim <= 0) return failmsg("initializer_set_resident: the device reports no LDS per workgroup");
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_init_sweep<InitSweepOptReg>), hipFuncAttributeMaxDynamicSharedMemorySize, lim));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_init_sweep<InitSweepResetTop>), hipFuncAttributeMaxDynamicSharedMemorySize, lim));
  R->lds_limit = (size_t)lim;
  return 0;
}

template <class BODY>
static int resSweep(DmvInitResident* R, hipStream_t s, const BODY& body) {
  if (R->n == 0) return 0;
  hipLaunchKernelGGL(k_init_sweep<BODY>, dim3(1), dim3(64), resSweepLds(R->n), s, R->n, R->levels, R->i(R->o_lbegin), R->i(R->o_order), R->i(R->o_nb), R->f(R->o_iR),
                     R->b(R->o_good), body);
  HIPCHK(hipGetLastError());
  R->work.launches++;
  return 0;
}
static int resOptReg(DmvInitResident* R, hipStream_t s, float regWeight) {
  InitSweepOptReg body;
  body.regWeight = regWeight; body.idepth = R->f(R->o_idepth);
  return resSweep(R, s, body);
}

// the slab of a point set of n points with `levels` sweep levels and n_listed parents listed: layout set, memory reserved, the pinned side free to write.  The handle is
// left WITHOUT resident state until the caller sets `live` (a HIP failure on the way leaves no half of one).
static int resBegin(DmvInitResident* R, int n, int levels, int n_listed, hipStream_t s) {
  DmvCursor L;
  DmvInitResidentLayout N;
  N.o_u = L.take<float>(n); N.o_v = L.take<float>(n); N.o_oth = L.take<float>(n); N.o_nb = L.take<int>(10 * (size_t)n); N.o_parent = L.take<int>(n);
  N.o_order = L.take<int>(n); N.o_lbegin = L.take<int>((size_t)levels + 1); N.o_cbegin = L.take<int>((size_t)n_listed + 1); N.o_children = L.take<int>(n);
  N.o_idepth = L.take<float>(n); N.o_iR = L.take<float>(n); N.o_lh = L.take<float>(n); N.o_energy = L.take<float>(2 * (size_t)n); N.o_good = L.take<unsigned char>(n);
  N.up_end = L.bytes();
  N.o_idn = L.take<float>(n); N.o_en_new = L.take<float>(2 * (size_t)n); N.o_maxstep = L.take<float>(n); N.o_lh_new = L.take<float>(n);
  N.o_jb[0] = L.take<float>(10 * (size_t)n); N.o_jb[1] = L.take<float>(10 * (size_t)n); N.o_good_new = L.take<unsigned char>(n);
  N.total = L.bytes();
  R->live = false;
  R->st.work = &R->work; R->io.work = &R->work;
  if (int r = R->st.reserve(N.total, N.total + N.total / 2, s)) return r;
  if (int r = R->st.begin(s)) return r;
  if (!R->io.d) {
    DmvCursor I;
    I.take<float>(RES_OUT_FLOATS); I.take<float>((size_t)INIT_EVAL_MAX_BLOCKS * IN_PART); I.take<float>((size_t)INIT_EVAL_MAX_BLOCKS * IN_EC);
    if (int r = R->io.create(I.bytes())) return r;
  }
  static_cast<DmvInitResidentLayout&>(*R) = N;
  return 0;
}

extern "C" {

int dmvio_hip_initializer_set_resident(dmvio_hip_initializer* m, int n, const float* u, const float* v, const float* idepth, const float* iR, const unsigned char* isGood,
                                       const float* energy2, const float* outlierTH, const float* lastHessian, const int* neighbours10, const int* parent) {
  static const char* who = "initializer_set_resident";
  if (!m) return failmsg("initializer_set_resident: null initializer handle");
  HIPCHK(hipSetDevice(m->ctx->device));
  dmvio_hip_ctx* c = m->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  char msg[256];
  if (n < 0 || n > m->capacity) { snprintf(msg, sizeof(msg), "%s: n = %d outside [0, %d], the handle's capacity", who, n, m->capacity); return failmsg(msg); }
  if (!u || !v || !idepth || !iR || !isGood || !energy2 || !outlierTH || !lastHessian || !neighbours10) return failmsg(std::string(who) + ": null array");
  for (size_t k = 0; k < 10 * (size_t)n; k++) {
    const int j = neighbours10[k];
    if (j != -1 && (j < 0 || j >= n)) { snprintf(msg, sizeof(msg), "%s: neighbour %d of point %d is %d: neither -1 nor in [0, %d)", who, (int)(k % 10), (int)(k / 10), j, n); return failmsg(msg); }
  }
  int max_parent = -1;
  if (parent) {
    const long long most = (long long)c->w * c->h;   // a level holds at most one point per pixel
    for (int i = 0; i < n; i++) {
      if (parent[i] < 0 || parent[i] >= most) { snprintf(msg, sizeof(msg), "%s: parent of point %d is %d: outside [0, %lld)", who, i, parent[i], most); return failmsg(msg); }
      max_parent = std::max(max_parent, parent[i]);
    }
  }
  if (!m->resident) m->resident = new DmvInitResident();
  DmvInitResident* R = m->resident;
  if (int r = resAllowLds(R, c->device)) return r;
  if (5 * (size_t)n > R->lds_limit) {
    snprintf(msg, sizeof(msg), "%s: n = %d points need %zu bytes of LDS for the ordered sweeps, the device allows a workgroup %zu (at most %zu points)", who, n, 5 * (size_t)n,
             R->lds_limit, R->lds_limit / 5);
    return failmsg(msg);
  }
  std::vector<int> level_begin, order, child_begin, children;
  const int levels = initSweepSchedule(n, neighbours10, level_begin, order);
  const int n_listed = parent ? max_parent + 1 : 0;
  if (parent) initChildLists(n, parent, n_listed, child_begin, children);
  hipStream_t s = c->stream;
  if (int r = resBegin(R, n, levels, n_listed, s)) return r;
  resOpen(R);
  char* h = R->st.host<char>(0);
  auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) memcpy(h + off, src, bytes); };
  const size_t F = sizeof(float) * (size_t)n, I4 = sizeof(int) * (size_t)n;
  put(R->o_u, u, F); put(R->o_v, v, F); put(R->o_oth, outlierTH, F); put(R->o_nb, neighbours10, 10 * I4);
  if (parent) put(R->o_parent, parent, I4);
  put(R->o_order, order.data(), I4); put(R->o_lbegin, level_begin.data(), sizeof(int) * level_begin.size());
  if (parent) { put(R->o_cbegin, child_begin.data(), sizeof(int) * child_begin.size()); put(R->o_children, children.data(), I4); }
  put(R->o_idepth, idepth, F); put(R->o_iR, iR, F); put(R->o_lh, lastHessian, F); put(R->o_energy, energy2, 2 * F); put(R->o_good, isGood, (size_t)n);
  R->n = n; R->levels = levels; R->n_listed = n_listed; R->max_parent = max_parent; R->has_parent = parent != nullptr; R->cur = 0;
  // ONE upload; the fields the caller does not give start zeroed, idepth_new = idepth (device to device).  No wait: stream-ordered.
  if (R->up_end) if (int r = R->st.upload(s, R->up_end)) return r;
  if (R->total > R->up_end) HIPCHK(hipMemsetAsync(R->st.d + R->up_end, 0, R->total - R->up_end, s));
  if (n) HIPCHK(hipMemcpyAsync(R->f(R->o_idn), R->f(R->o_idepth), F, hipMemcpyDeviceToDevice, s));
  R->live = true;
  return 0;
}

int dmvio_hip_initializer_resident_reset_unsnapped(dmvio_hip_initializer* m) {
  RES_HEAD(m, "initializer_resident_reset_unsnapped");
  resOpen(R);
  if (R->n == 0) return 0;
  hipLaunchKernelGGL(k_init_reset_unsnapped, resGrid(R->n), dim3(256), 0, s, R->n, R->f(R->o_iR), R->f(R->o_idn), R->f(R->o_lh));
  HIPCHK(hipGetLastError());
  R->work.launches++;
  return 0;
}

int dmvio_hip_initializer_resident_reset_points(dmvio_hip_initializer* m, int is_top_level) {
  RES_HEAD(m, "initializer_resident_reset_points");
  resOpen(R);
  if (R->n == 0) return 0;
  hipLaunchKernelGGL(k_init_reset_points, resGrid(R->n), dim3(256), 0, s, R->n, R->f(R->o_idepth), R->f(R->o_idn), R->f(R->o_energy));
  HIPCHK(hipGetLastError());
  R->work.launches++;
  if (!is_top_level) return 0;
  // (the reference's one loop does both per point; the fields of the first part are read by no other point's second part, so all first parts may go first)
  InitSweepResetTop body;
  body.idepth = R->f(R->o_idepth); body.idepth_new = R->f(R->o_idn);
  return resSweep(R, s, body);
}

int dmvio_hip_initializer_resident_do_step(dmvio_hip_initializer* m, float lambda, const float inc8[8]) {
  RES_HEAD(m, "initializer_resident_do_step");
  if (!inc8) return failmsg("initializer_resident_do_step: null inc8");
  resOpen(R);
  if (R->n == 0) return 0;
  InitInc8 inc;
  for (int k = 0; k < 8; k++) inc.v[k] = inc8[k];
  hipLaunchKernelGGL(k_init_do_step, resGrid(R->n), dim3(256), 0, s, R->n, lambda, inc, R->b(R->o_good), R->f(R->o_jb[R->cur]), R->f(R->o_maxstep), R->f(R->o_idepth),
                     R->f(R->o_idn));
  HIPCHK(hipGetLastError());
  R->work.launches++;
  return 0;
}

int dmvio_hip_initializer_resident_apply_step(dmvio_hip_initializer* m) {
  RES_HEAD(m, "initializer_resident_apply_step");
  resOpen(R);
  if (R->n) {
    hipLaunchKernelGGL(k_init_apply_step, resGrid(R->n), dim3(256), 0, s, R->n, R->b(R->o_good), R->b(R->o_good_new), R->f(R->o_idepth), R->f(R->o_idn), R->f(R->o_iR),
                       R->f(R->o_energy), R->f(R->o_en_new), R->f(R->o_lh), R->f(R->o_lh_new));
    HIPCHK(hipGetLastError());
    R->work.launches++;
  }
  R->cur ^= 1;   // std::swap(JbBuffer, JbBuffer_new) (:964)
  return 0;
}

int dmvio_hip_initializer_resident_opt_reg(dmvio_hip_initializer* m, float regWeight) {
  RES_HEAD(m, "initializer_resident_opt_reg");
  resOpen(R);
  return resOptReg(R, s, regWeight);
}

}  // extern "C"

// what both propagate calls refuse; lo: the lower level (it names its parents), hi: the upper one
static int resPropagateHead(const char* who, dmvio_hip_initializer* lo, dmvio_hip_initializer* hi) {
  char msg[256];
  for (dmvio_hip_initializer* m : {lo, hi})
    if (!m->resident || !m->resident->live) { snprintf(msg, sizeof(msg), "%s: a handle has no resident point set (dmvio_hip_initializer_set_resident)", who); return failmsg(msg); }
  if (lo == hi) { snprintf(msg, sizeof(msg), "%s: the same handle named as both levels", who); return failmsg(msg); }
  if (!lo->resident->has_parent) { snprintf(msg, sizeof(msg), "%s: the lower level was set without a parent table", who); return failmsg(msg); }
  if (lo->resident->max_parent >= hi->resident->n) {
    snprintf(msg, sizeof(msg), "%s: the lower level names parent %d, the upper level has %d points", who, lo->resident->max_parent, hi->resident->n);
    return failmsg(msg);
  }
  return 0;
}

extern "C" {

int dmvio_hip_initializer_resident_propagate_down(dmvio_hip_initializer* src, dmvio_hip_initializer* dst, float regWeight, int snapped) {
  static const char* who = "initializer_resident_propagate_down";
  if (!src || !dst) return failmsg("initializer_resident_propagate_down: null initializer handle");
  if (src->ctx != dst->ctx) return failmsg("initializer_resident_propagate_down: the two handles belong to different contexts");
  HIPCHK(hipSetDevice(dst->ctx->device));
  dmvio_hip_ctx* c = dst->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (int r = resPropagateHead(who, dst, src)) return r;
  DmvInitResident *U = src->resident, *R = dst->resident;
  hipStream_t s = c->stream;
  resOpen(R);
  if (R->n) {
    hipLaunchKernelGGL(k_init_propagate_down, resGrid(R->n), dim3(256), 0, s, R->n, R->i(R->o_parent), U->b(U->o_good), U->f(U->o_iR), U->f(U->o_lh), R->b(R->o_good),
                       R->f(R->o_iR), R->f(R->o_idepth), R->f(R->o_idn), R->f(R->o_lh));
    HIPCHK(hipGetLastError());
    R->work.launches++;
  }
  return snapped ? resOptReg(R, s, regWeight) : 0;
}

int dmvio_hip_initializer_resident_propagate_up(dmvio_hip_initializer* src, dmvio_hip_initializer* dst, float regWeight, int snapped) {
  static const char* who = "initializer_resident_propagate_up";
  if (!src || !dst) return failmsg("initializer_resident_propagate_up: null initializer handle");
  if (src->ctx != dst->ctx) return failmsg("initializer_resident_propagate_up: the two handles belong to different contexts");
  HIPCHK(hipSetDevice(dst->ctx->device));
  dmvio_hip_ctx* c = dst->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (int r = resPropagateHead(who, src, dst)) return r;
  DmvInitResident *Lo = src->resident, *R = dst->resident;
  hipStream_t s = c->stream;
  resOpen(R);
  if (R->n) {
    hipLaunchKernelGGL(k_init_propagate_up, resGrid(R->n), dim3(256), 0, s, R->n, Lo->n_listed, Lo->i(Lo->o_cbegin), Lo->i(Lo->o_children), Lo->b(Lo->o_good), Lo->f(Lo->o_iR),
                       Lo->f(Lo->o_lh), R->f(R->o_iR), R->f(R->o_idepth), R->b(R->o_good));
    HIPCHK(hipGetLastError());
    R->work.launches++;
  }
  return snapped ? resOptReg(R, s, regWeight) : 0;
}

int dmvio_hip_initializer_resident_calc(dmvio_hip_initializer* m, int lvl, int first_slot, int new_slot, const double Ki9[9], const float fxfycxcy_lvl[4],
                                        const double refToNew7[7], const double aff_ab[2], float alphaW, float alphaK, float couplingWeight, double priorY, double priorX,
                                        int snapped, float* H_out64, float* b_out8, float* H_sc64, float* b_sc8, float res3[3], float* ec3) {
  RES_HEAD(m, "initializer_resident_calc");
  if (!Ki9 || !fxfycxcy_lvl || !refToNew7 || !aff_ab || !H_out64 || !b_out8 || !H_sc64 || !b_sc8 || !res3) return failmsg("initializer_resident_calc: null argument");
  if (lvl < 0 || lvl >= c->levels || first_slot < 0 || first_slot >= c->n_slots || new_slot < 0 || new_slot >= c->n_slots)
    return failmsg("initializer_resident_calc: level / slot out of range");
  const int n = R->n;
  resOpen(R);
  // the range check.  The host copy of (u, v) says whether ANY point could leave the level; only then does isGood, which lives on the device, matter — and it is asked
  // BEFORE the evaluation, which reads the image around every good point without a test.
  {
    const float *hu = R->st.host<float>(R->o_u), *hv = R->st.host<float>(R->o_v);
    const float umax = (float)(c->wl[lvl] - 3), vmax = (float)(c->hl[lvl] - 3);
    int first = -1;
    for (int i = 0; i < n && first < 0; i++)
      if (!(hu[i] >= 2.0f && hu[i] < umax && hv[i] >= 2.0f && hv[i] < vmax)) first = i;
    if (first >= 0) {
      int* d_count = R->io.dev<int>(sizeof(float) * RES_COUNT);
      HIPCHK(hipMemsetAsync(d_count, 0, sizeof(int), s));
      hipLaunchKernelGGL(k_init_count_outside, resGrid(n), dim3(256), 0, s, n, R->b(R->o_good), R->f(R->o_u), R->f(R->o_v), umax, vmax, d_count);
      HIPCHK(hipGetLastError());
      R->work.launches++;
      if (int r = R->io.download(s, sizeof(float) * RES_COUNT, sizeof(int))) return r;
      if (int r = R->io.wait(s)) return r;
      const int outside = *R->io.host<int>(sizeof(float) * RES_COUNT);
      if (outside) {
        char msg[256];
        snprintf(msg, sizeof(msg), "initializer_resident_calc: %d good point(s) outside [2, %d) x [2, %d) of level %d (the first point outside, good or not, is %d at (%g, %g))",
                 outside, c->wl[lvl] - 3, c->hl[lvl] - 3, lvl, first, (double)hu[first], (double)hv[first]);
        R->work_closed = true;
        return failmsg(msg);
      }
    }
  }
  if (lvl == 0) { if (int r = dmv_ensure_row_major_locked(c, first_slot)) return r; if (int r = dmv_ensure_row_major_locked(c, new_slot)) return r; }
  const Pose T = poseFrom7(refToNew7);
  const InitArgs A = initMakeArgs(c, lvl, Ki9, fxfycxcy_lvl, T, aff_ab, n, alphaW, alphaK, couplingWeight);
  InitPts P;
  P.n = n; P.u = R->f(R->o_u); P.v = R->f(R->o_v); P.idepth_new = R->f(R->o_idn); P.iR = R->f(R->o_iR); P.energy = R->f(R->o_energy); P.outlierTH = R->f(R->o_oth);
  P.isGood = R->b(R->o_good);
  P.energy_new = R->f(R->o_en_new); P.maxstep = R->f(R->o_maxstep); P.lastHessian_new = R->f(R->o_lh_new); P.JbBuffer_new = R->f(R->o_jb[R->cur ^ 1]);
  P.isGood_new = R->b(R->o_good_new);
  float* d_out = R->io.dev<float>(0);
  float* d_part = d_out + RES_OUT_FLOATS;
  float* d_ecpart = d_part + (size_t)INIT_EVAL_MAX_BLOCKS * IN_PART;
  if (int r = initLaunchEval(c, lvl, first_slot, new_slot, P, A, d_part, d_out)) return r;
  R->work.launches += 2;
  const bool ec = ec3 && snapped;
  if (ec) {   // calcEC behind the evaluation: it reads isGood_new
    const int G = initEvalGrid(n);
    hipLaunchKernelGGL(k_init_ec, dim3(G), dim3(256), 0, s, n, R->b(R->o_good_new), R->f(R->o_idepth), R->f(R->o_idn), R->f(R->o_iR), d_ecpart);
    hipLaunchKernelGGL(k_init_ec_final, dim3(1), dim3(64), 0, s, G, d_ecpart, d_out + RES_EC);
    HIPCHK(hipGetLastError());
    R->work.launches += 2;
  }
  if (int r = R->io.download(s, 0, sizeof(float) * RES_DOWN)) return r;
  if (int r = R->io.wait(s)) return r;
  R->st.settled();
  R->work_closed = true;
  const float* out = R->io.host<float>(0);
  initHostTail(T, n, alphaW, alphaK, priorY, priorX, out, H_out64, b_out8, H_sc64, b_sc8, res3);
  if (ec3) {
    if (ec) { ec3[0] = couplingWeight * out[RES_EC]; ec3[1] = couplingWeight * out[RES_EC + 1]; ec3[2] = out[RES_EC + 2]; }
    else { ec3[0] = 0; ec3[1] = 0; ec3[2] = (float)n; }   // (:652)
  }
  return 0;
}

int dmvio_hip_initializer_resident_get_state(dmvio_hip_initializer* m, float* idepth, float* iR, unsigned char* isGood, float* energy2, float* lastHessian,
                                             float* idepth_new, unsigned char* isGood_new, float* energy_new2, float* lastHessian_new, float* maxstep, float* JbBuffer10) {
  RES_HEAD(m, "initializer_resident_get_state");
  resOpen(R);
  const int n = R->n;
  // (stream order puts this download behind set_resident's upload from the same pinned memory)
  if (R->total > R->o_idepth) if (int r = R->st.download(s, R->o_idepth, R->total - R->o_idepth)) return r;
  if (int r = R->st.wait(s)) return r;
  R->work_closed = true;
  const char* h = R->st.host<char>(0);
  auto get = [&](void* dst, size_t off, size_t bytes) { if (dst && bytes) memcpy(dst, h + off, bytes); };
  const size_t F = sizeof(float) * (size_t)n;
  get(idepth, R->o_idepth, F); get(iR, R->o_iR, F); get(isGood, R->o_good, (size_t)n); get(energy2, R->o_energy, 2 * F); get(lastHessian, R->o_lh, F);
  get(idepth_new, R->o_idn, F); get(isGood_new, R->o_good_new, (size_t)n); get(energy_new2, R->o_en_new, 2 * F); get(lastHessian_new, R->o_lh_new, F);
  get(maxstep, R->o_maxstep, F); get(JbBuffer10, R->o_jb[R->cur], 10 * F);
  return 0;
}

int dmvio_hip_initializer_resident_set_state(dmvio_hip_initializer* m, const float* idepth, const float* iR, const unsigned char* isGood, const float* energy2,
                                             const float* lastHessian, const float* idepth_new, const unsigned char* isGood_new, const float* energy_new2,
                                             const float* lastHessian_new, const float* maxstep, const float* JbBuffer10, const float* JbBuffer_new10) {
  RES_HEAD(m, "initializer_resident_set_state");
  resOpen(R);
  const int n = R->n;
  if (R->st.busy()) { if (int r = R->st.begin(s)) return r; }   // the pinned side may still be read by an earlier upload
  char* h = R->st.host<char>(0);
  const size_t F = sizeof(float) * (size_t)n;
  const struct { const void* src; size_t off, bytes; } part[12] = {
      {idepth, R->o_idepth, F}, {iR, R->o_iR, F}, {isGood, R->o_good, (size_t)n}, {energy2, R->o_energy, 2 * F}, {lastHessian, R->o_lh, F}, {idepth_new, R->o_idn, F},
      {isGood_new, R->o_good_new, (size_t)n}, {energy_new2, R->o_en_new, 2 * F}, {lastHessian_new, R->o_lh_new, F}, {maxstep, R->o_maxstep, F},
      {JbBuffer10, R->o_jb[R->cur], 10 * F}, {JbBuffer_new10, R->o_jb[R->cur ^ 1], 10 * F}};
  bool any = false;
  for (const auto& q : part) {
    if (!q.src || !q.bytes) continue;
    memcpy(h + q.off, q.src, q.bytes);
    HIPCHK(hipMemcpyAsync(R->st.d + q.off, h + q.off, q.bytes, hipMemcpyHostToDevice, s));
    R->work.uploads++;
    any = true;
  }
  if (any) R->st.in_flight[R->st.cur] = true;   // (the next writer of the pinned side waits, as behind DmvSlab::upload)
  return 0;
}

int dmvio_hip_initializer_resident_last_work(dmvio_hip_initializer* m, int* launches, int* uploads, int* downloads, int* waits) {
  RES_HEAD(m, "initializer_resident_last_work");
  R->work.report(launches, uploads, downloads, waits);
  return 0;
}

}  // extern "C"

// ---- for dmvio_hip_initializer_set_first (capi_init_first.hip; declared in init_handle.h).  The caller holds the context's lock.
// what set_resident would refuse of n points on this handle, without touching the handle: 0 or <0 with the message
int dmvInitResidentCheck(dmvio_hip_initializer* m, int n, const char* who) {
  char msg[256];
  if (n < 0 || n > m->capacity) { snprintf(msg, sizeof(msg), "%s: n = %d outside [0, %d], the handle's capacity", who, n, m->capacity); return failmsg(msg); }
  int lim = 0;
  HIPCHK(hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, m->ctx->device));
  if (5 * (size_t)n > (size_t)std::max(lim, 0)) {
    snprintf(msg, sizeof(msg), "%s: n = %d points need %zu bytes of LDS for the ordered sweeps, the device allows a workgroup %zu (at most %zu points)", who, n, 5 * (size_t)n,
             (size_t)std::max(lim, 0), (size_t)std::max(lim, 0) / 5);
    return failmsg(msg);
  }
  return 0;
}
// The state set_resident leaves when given setFirst's arrays (idepth = iR = 1, isGood = 1, energy = lastHessian = 0, outlierTH constant), from point lists on the device
// (d_*) of which the host holds a copy (h_*; parent NULL on the top level): the sweep schedule and the children lists are built here from the host copy and are the ONE
// upload; no point value is uploaded.  The caller has run dmvInitResidentCheck and checked the tables' ranges.
int dmvInitResidentAdopt(dmvio_hip_initializer* m, int n, const float* d_u, const float* d_v, const int* d_nb, const int* d_parent, const float* h_u, const float* h_v,
                         const int* h_nb, const int* h_parent, float outlierTH, DmvWork* work) {
  dmvio_hip_ctx* c = m->ctx;
  hipStream_t s = c->stream;
  int max_parent = -1;
  if (h_parent) for (int i = 0; i < n; i++) max_parent = std::max(max_parent, h_parent[i]);
  if (!m->resident) m->resident = new DmvInitResident();
  DmvInitResident* R = m->resident;
  if (int r = resAllowLds(R, c->device)) return r;
  std::vector<int> level_begin, order, child_begin, children;
  const int levels = initSweepSchedule(n, h_nb, level_begin, order);
  const int n_listed = h_parent ? max_parent + 1 : 0;
  if (h_parent) initChildLists(n, h_parent, n_listed, child_begin, children);
  if (int r = resBegin(R, n, levels, n_listed, s)) return r;
  resOpen(R);
  char* h = R->st.host<char>(0);
  auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) memcpy(h + off, src, bytes); };
  const size_t F = sizeof(float) * (size_t)n, I4 = sizeof(int) * (size_t)n;
  put(R->o_u, h_u, F); put(R->o_v, h_v, F);   // the host copy of (u, v) the range check of calc reads
  put(R->o_order, order.data(), I4); put(R->o_lbegin, level_begin.data(), sizeof(int) * level_begin.size());
  if (h_parent) { put(R->o_cbegin, child_begin.data(), sizeof(int) * child_begin.size()); put(R->o_children, children.data(), I4); }
  R->n = n; R->levels = levels; R->n_listed = n_listed; R->max_parent = max_parent; R->has_parent = h_parent != nullptr; R->cur = 0;
  // the tables lie back to back between the static point arrays and the dynamic part: one copy
  HIPCHK(hipMemcpyAsync(R->st.d + R->o_order, h + R->o_order, R->o_idepth - R->o_order, hipMemcpyHostToDevice, s));
  R->st.in_flight[R->st.cur] = true;   // (the next writer of the pinned side waits, as behind DmvSlab::upload)
  R->work.uploads++; if (work) work->uploads++;
  HIPCHK(hipMemsetAsync(R->st.d + R->o_idepth, 0, R->total - R->o_idepth, s));
  hipLaunchKernelGGL(k_init_adopt, resGrid(n), dim3(256), 0, s, n, d_u, d_v, d_nb, d_parent, outlierTH, R->f(R->o_u), R->f(R->o_v), R->f(R->o_oth), R->i(R->o_nb),
                     R->i(R->o_parent), R->f(R->o_idepth), R->f(R->o_iR), R->f(R->o_idn), R->b(R->o_good));
  HIPCHK(hipGetLastError());
  R->work.launches++; if (work) work->launches++;
  R->live = true;
  return 0;
}
