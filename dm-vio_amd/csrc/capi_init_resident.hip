// C ABI of the resident initializer (include/dmvio_hip_init_resident.h): the point set of a level and both JbBuffers in device memory, and the per-point passes of
// CoarseInitializer::trackFrame (src/dso/FullSystem/CoarseInitializer.cpp) on them.  The evaluation is capi_init.hip's (initLaunchEval): the same kernels on the same grid.
// This unit also installs the point set for both of its sources — the caller's arrays (set_resident) and setFirst's lists on the device (dmvInitResidentAdopt) — and holds
// the one copy of the launches the LM unit enqueues too (init_resident_state.h).
#include <vector>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <algorithm>
#include "../../include/dmvio_hip_init_resident.h"
#include "init_resident_state.h"   // the handle, the resident state, its layout and the two host tables (init_resident_host.hpp)
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
// one launch on stream s, checked, and counted into `work` where there is one
#define RES_LAUNCH(work, kernel, grid, block, lds, s, ...)        \
  do {                                                            \
    hipLaunchKernelGGL(kernel, grid, block, lds, s, __VA_ARGS__); \
    HIPCHK(hipGetLastError());                                    \
    if (DmvWork* w_ = (work)) w_->launches++;                     \
  } while (0)

template <class BODY>
static int resSweep(DmvInitResident* R, hipStream_t s, const BODY& body) {
  if (R->n == 0) return 0;
  RES_LAUNCH(&R->work, k_init_sweep<BODY>, dim3(1), dim3(64), resSweepLds(R->n), s, R->n, R->levels, R->i(R->o_lbegin), R->i(R->o_order), R->i(R->o_nb), R->f(R->o_iR),
             R->b(R->o_good), body);
  return 0;
}
static int resOptReg(DmvInitResident* R, hipStream_t s, float regWeight) {
  InitSweepOptReg body;
  body.regWeight = regWeight; body.idepth = R->f(R->o_idepth);
  return resSweep(R, s, body);
}

// ---- the launches capi_init_lm.hip enqueues too (declared in init_resident_state.h)
int resPropagateDown(DmvInitResident* R, const DmvInitResident* U, hipStream_t s, DmvWork* work) {
  if (R->n == 0) return 0;
  RES_LAUNCH(work, k_init_propagate_down, resGrid(R->n), dim3(256), 0, s, R->n, R->i(R->o_parent), U->b(U->o_good), U->f(U->o_iR), U->f(U->o_lh), R->b(R->o_good),
             R->f(R->o_iR), R->f(R->o_idepth), R->f(R->o_idn), R->f(R->o_lh));
  return 0;
}
int resPropagateUp(DmvInitResident* R, const DmvInitResident* Lo, hipStream_t s, DmvWork* work) {
  if (R->n == 0) return 0;
  RES_LAUNCH(work, k_init_propagate_up, resGrid(R->n), dim3(256), 0, s, R->n, Lo->n_listed, Lo->i(Lo->o_cbegin), Lo->i(Lo->o_children), Lo->b(Lo->o_good), Lo->f(Lo->o_iR),
             Lo->f(Lo->o_lh), R->f(R->o_iR), R->f(R->o_idepth), R->b(R->o_good));
  return 0;
}
int resCountOutside(DmvInitResident* R, int wl, int hl, hipStream_t s, DmvWork* work, int* outside) {
  const size_t at = sizeof(float) * RES_COUNT;
  HIPCHK(hipMemsetAsync(R->io.dev<int>(at), 0, sizeof(int), s));
  RES_LAUNCH(work, k_init_count_outside, resGrid(R->n), dim3(256), 0, s, R->n, R->b(R->o_good), R->f(R->o_u), R->f(R->o_v), (float)(wl - 3), (float)(hl - 3), R->io.dev<int>(at));
  R->io.work = work;   // (the slab counts its download and its wait into R->work otherwise)
  int r = R->io.download(s, at, sizeof(int));
  if (!r) r = R->io.wait(s);
  R->io.work = &R->work;
  *outside = *R->io.host<int>(at);
  return r;
}

// the two size refusals of a point set: the handle's capacity, and the LDS the ordered sweeps need against the device's limit (lds_limit)
static int resSizeCheck(const dmvio_hip_initializer* m, int n, size_t lds_limit, const char* who) {
  char msg[256];
  if (n < 0 || n > m->capacity) { snprintf(msg, sizeof(msg), "%s: n = %d outside [0, %d], the handle's capacity", who, n, m->capacity); return failmsg(msg); }
  if (5 * (size_t)n > lds_limit) {
    snprintf(msg, sizeof(msg), "%s: n = %d points need %zu bytes of LDS for the ordered sweeps, the device allows a workgroup %zu (at most %zu points)", who, n, 5 * (size_t)n,
             lds_limit, lds_limit / 5);
    return failmsg(msg);
  }
  return 0;
}

// The ONE way a handle gets a resident point set — dmvio_hip_initializer_set_resident from the caller's arrays, dmvInitResidentAdopt from setFirst's lists: the size
// refusals, the state object, the LDS allowance of the sweeps, the sweep schedule and the child lists from the host's tables (h_parent NULL: the top level), the slab laid
// out for them with its pinned side free to write, the tables and the host copy of (u, v) in the pinned side, and the scalar fields.  Nothing is enqueued and `live` is
// left false: the caller fills the point arrays and sets it (a HIP failure on the way leaves no half of a point set).
static int resInstall(dmvio_hip_initializer* m, int n, const float* h_u, const float* h_v, const int* h_nb, const int* h_parent, const char* who, DmvInitResident** out) {
  dmvio_hip_ctx* c = m->ctx;
  hipStream_t s = c->stream;
  if (!m->resident) m->resident = new DmvInitResident();
  DmvInitResident* R = m->resident;
  if (!R->lds_limit) {
    int lim = 0;
    size_t own = 0;
    HIPCHK(initLdsAllow(c->device, &lim, reinterpret_cast<const void*>(&k_init_sweep<InitSweepOptReg>), &own));
    if (lim <= 0) return failmsg("initializer_set_resident: the device reports no LDS per workgroup");
    HIPCHK(initLdsAllow(c->device, &lim, reinterpret_cast<const void*>(&k_init_sweep<InitSweepResetTop>), &own));
    R->lds_limit = (size_t)lim;
  }
  if (int r = resSizeCheck(m, n, R->lds_limit, who)) return r;
  std::vector<int> level_begin, order, child_begin, children;
  const int levels = initSweepSchedule(n, h_nb, level_begin, order);
  int max_parent = -1;
  if (h_parent) for (int i = 0; i < n; i++) max_parent = std::max(max_parent, h_parent[i]);
  const int n_listed = h_parent ? max_parent + 1 : 0;
  if (h_parent) initChildLists(n, h_parent, n_listed, child_begin, children);
  const DmvInitResidentLayout N = initResidentLayout<DmvCursor>(n, levels, n_listed);
  R->live = false;
  R->st.work = &R->work; R->io.work = &R->work;
  if (int r = R->st.reserve(N.total, N.total + N.total / 2, s)) return r;
  if (int r = R->st.begin(s)) return r;
  if (!R->io.d) {
    DmvCursor I;
    I.take<float>(RES_OUT_FLOATS); I.take<float>((size_t)INIT_MAX_BLOCKS * IN_PART); I.take<float>((size_t)INIT_MAX_BLOCKS * IN_EC);
    if (int r = R->io.create(I.bytes())) return r;
  }
  static_cast<DmvInitResidentLayout&>(*R) = N;
  resOpen(R);
  const size_t I4 = sizeof(int) * (size_t)n;
  R->put(R->o_u, h_u, sizeof(float) * (size_t)n); R->put(R->o_v, h_v, sizeof(float) * (size_t)n);
  R->put(R->o_order, order.data(), I4); R->put(R->o_lbegin, level_begin.data(), sizeof(int) * level_begin.size());
  if (h_parent) { R->put(R->o_cbegin, child_begin.data(), sizeof(int) * child_begin.size()); R->put(R->o_children, children.data(), I4); }
  R->n = n; R->levels = levels; R->n_listed = n_listed; R->max_parent = max_parent; R->has_parent = h_parent != nullptr; R->cur = 0;
  *out = R;
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
  if (int r = resSizeCheck(m, n, ~(size_t)0, who)) return r;   // the capacity, in front of the tables' checks; the LDS once the install knows the limit
  if (!u || !v || !idepth || !iR || !isGood || !energy2 || !outlierTH || !lastHessian || !neighbours10) return failmsg(std::string(who) + ": null array");
  for (size_t k = 0; k < 10 * (size_t)n; k++) {
    const int j = neighbours10[k];
    if (j != -1 && (j < 0 || j >= n)) { snprintf(msg, sizeof(msg), "%s: neighbour %d of point %d is %d: neither -1 nor in [0, %d)", who, (int)(k % 10), (int)(k / 10), j, n); return failmsg(msg); }
  }
  if (parent) {
    const long long most = (long long)c->w * c->h;   // a level holds at most one point per pixel
    for (int i = 0; i < n; i++)
      if (parent[i] < 0 || parent[i] >= most) { snprintf(msg, sizeof(msg), "%s: parent of point %d is %d: outside [0, %lld)", who, i, parent[i], most); return failmsg(msg); }
  }
  DmvInitResident* R;
  if (int r = resInstall(m, n, u, v, neighbours10, parent, who, &R)) return r;
  hipStream_t s = c->stream;
  const size_t F = sizeof(float) * (size_t)n;
  R->put(R->o_oth, outlierTH, F); R->put(R->o_nb, neighbours10, 10 * sizeof(int) * (size_t)n);
  if (parent) R->put(R->o_parent, parent, sizeof(int) * (size_t)n);
  R->put(R->o_idepth, idepth, F); R->put(R->o_iR, iR, F); R->put(R->o_lh, lastHessian, F); R->put(R->o_energy, energy2, 2 * F); R->put(R->o_good, isGood, (size_t)n);
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
  RES_LAUNCH(&R->work, k_init_reset_unsnapped, resGrid(R->n), dim3(256), 0, s, R->n, R->f(R->o_iR), R->f(R->o_idn), R->f(R->o_lh));
  return 0;
}

int dmvio_hip_initializer_resident_reset_points(dmvio_hip_initializer* m, int is_top_level) {
  RES_HEAD(m, "initializer_resident_reset_points");
  resOpen(R);
  if (R->n == 0) return 0;
  RES_LAUNCH(&R->work, k_init_reset_points, resGrid(R->n), dim3(256), 0, s, R->n, R->f(R->o_idepth), R->f(R->o_idn), R->f(R->o_energy));
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
  RES_LAUNCH(&R->work, k_init_do_step, resGrid(R->n), dim3(256), 0, s, R->n, lambda, inc, R->b(R->o_good), R->f(R->o_jb[R->cur]), R->f(R->o_maxstep), R->f(R->o_idepth),
             R->f(R->o_idn));
  return 0;
}

int dmvio_hip_initializer_resident_apply_step(dmvio_hip_initializer* m) {
  RES_HEAD(m, "initializer_resident_apply_step");
  resOpen(R);
  if (R->n)
    RES_LAUNCH(&R->work, k_init_apply_step, resGrid(R->n), dim3(256), 0, s, R->n, R->b(R->o_good), R->b(R->o_good_new), R->f(R->o_idepth), R->f(R->o_idn), R->f(R->o_iR),
               R->f(R->o_energy), R->f(R->o_en_new), R->f(R->o_lh), R->f(R->o_lh_new));
  R->cur ^= 1;   // std::swap(JbBuffer, JbBuffer_new) (:964)
  return 0;
}

int dmvio_hip_initializer_resident_opt_reg(dmvio_hip_initializer* m, float regWeight) {
  RES_HEAD(m, "initializer_resident_opt_reg");
  resOpen(R);
  return resOptReg(R, s, regWeight);
}

}  // extern "C"

// both propagate calls: the refusals, the pass into dst and, where snapped, optReg behind it.  down: dst is the lower level (it names its parents), else the upper one
static int resPropagate(const char* who, bool down, dmvio_hip_initializer* src, dmvio_hip_initializer* dst, float regWeight, int snapped) {
  char msg[256];
  auto no = [&](const char* what) { snprintf(msg, sizeof(msg), "%s: %s", who, what); return failmsg(msg); };
  if (!src || !dst) return no("null initializer handle");
  if (src->ctx != dst->ctx) return no("the two handles belong to different contexts");
  HIPCHK(hipSetDevice(dst->ctx->device));
  dmvio_hip_ctx* c = dst->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  dmvio_hip_initializer *lo = down ? dst : src, *hi = down ? src : dst;
  for (dmvio_hip_initializer* m : {lo, hi})
    if (!m->resident || !m->resident->live) return no("a handle has no resident point set (dmvio_hip_initializer_set_resident)");
  if (lo == hi) return no("the same handle named as both levels");
  if (!lo->resident->has_parent) return no("the lower level was set without a parent table");
  if (lo->resident->max_parent >= hi->resident->n) {
    snprintf(msg, sizeof(msg), "%s: the lower level names parent %d, the upper level has %d points", who, lo->resident->max_parent, hi->resident->n);
    return failmsg(msg);
  }
  DmvInitResident* R = dst->resident;
  hipStream_t s = c->stream;
  resOpen(R);
  if (int r = down ? resPropagateDown(R, src->resident, s, &R->work) : resPropagateUp(R, src->resident, s, &R->work)) return r;
  return snapped ? resOptReg(R, s, regWeight) : 0;
}

extern "C" {

int dmvio_hip_initializer_resident_propagate_down(dmvio_hip_initializer* src, dmvio_hip_initializer* dst, float regWeight, int snapped) {
  return resPropagate("initializer_resident_propagate_down", true, src, dst, regWeight, snapped);
}
int dmvio_hip_initializer_resident_propagate_up(dmvio_hip_initializer* src, dmvio_hip_initializer* dst, float regWeight, int snapped) {
  return resPropagate("initializer_resident_propagate_up", false, src, dst, regWeight, snapped);
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
  const int first = resFirstOutside(R, c->wl[lvl], c->hl[lvl]);
  if (first >= 0) {
    int outside = 0;
    if (int r = resCountOutside(R, c->wl[lvl], c->hl[lvl], s, &R->work, &outside)) return r;
    if (outside) {
      char msg[256];
      snprintf(msg, sizeof(msg), "initializer_resident_calc: %d good point(s) outside [2, %d) x [2, %d) of level %d (the first point outside, good or not, is %d at (%g, %g))",
               outside, c->wl[lvl] - 3, c->hl[lvl] - 3, lvl, first, (double)R->st.host<float>(R->o_u)[first], (double)R->st.host<float>(R->o_v)[first]);
      R->work_closed = true;
      return failmsg(msg);
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
  float* d_ecpart = d_part + (size_t)INIT_MAX_BLOCKS * IN_PART;
  if (int r = initLaunchEval(c, lvl, first_slot, new_slot, P, A, d_part, d_out)) return r;
  R->work.launches += 2;
  const bool ec = ec3 && snapped;
  if (ec) {   // calcEC behind the evaluation: it reads isGood_new
    const int G = initGrid(n);
    RES_LAUNCH(&R->work, k_init_ec, dim3(G), dim3(256), 0, s, n, R->b(R->o_good_new), R->f(R->o_idepth), R->f(R->o_idn), R->f(R->o_iR), d_ecpart);
    RES_LAUNCH(&R->work, k_init_ec_final, dim3(1), dim3(64), 0, s, G, d_ecpart, d_out + RES_EC);
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
// what the install refuses of n points on this handle, without touching the handle: 0 or <0 with the message
int dmvInitResidentCheck(dmvio_hip_initializer* m, int n, const char* who) {
  int lim = 0;
  HIPCHK(initLdsAllow(m->ctx->device, &lim));
  return resSizeCheck(m, n, (size_t)std::max(lim, 0), who);
}
// The state set_resident leaves when given setFirst's arrays (idepth = iR = 1, isGood = 1, energy = lastHessian = 0, outlierTH constant), from point lists on the device
// (d_*) of which the host holds a copy (h_*; parent NULL on the top level): the tables the install builds from the host copy are the ONE upload; no point value is
// uploaded.  The caller has run dmvInitResidentCheck and checked the tables' ranges.
int dmvInitResidentAdopt(dmvio_hip_initializer* m, int n, const float* d_u, const float* d_v, const int* d_nb, const int* d_parent, const float* h_u, const float* h_v,
                         const int* h_nb, const int* h_parent, float outlierTH, DmvWork* work) {
  hipStream_t s = m->ctx->stream;
  DmvInitResident* R;
  if (int r = resInstall(m, n, h_u, h_v, h_nb, h_parent, "initializer_set_first", &R)) return r;
  // the tables lie back to back between the static point arrays and the dynamic part (initResidentLayout; tests/init_sweep_harness.cpp holds it to that): one copy
  HIPCHK(hipMemcpyAsync(R->st.d + R->o_order, R->st.host<char>(R->o_order), R->o_idepth - R->o_order, hipMemcpyHostToDevice, s));
  R->st.in_flight[R->st.cur] = true;   // (the next writer of the pinned side waits, as behind DmvSlab::upload)
  R->work.uploads++; if (work) work->uploads++;
  HIPCHK(hipMemsetAsync(R->st.d + R->o_idepth, 0, R->total - R->o_idepth, s));
  RES_LAUNCH(&R->work, k_init_adopt, resGrid(n), dim3(256), 0, s, n, d_u, d_v, d_nb, d_parent, outlierTH, R->f(R->o_u), R->f(R->o_v), R->f(R->o_oth), R->i(R->o_nb),
             R->i(R->o_parent), R->f(R->o_idepth), R->f(R->o_iR), R->f(R->o_idn), R->b(R->o_good));
  if (work) work->launches++;
  R->live = true;
  return 0;
}
