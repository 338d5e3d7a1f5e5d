// C ABI of the initializer's LM loop on the device (include/dmvio_hip_init_lm.h): CoarseInitializer::trackFrame (src/dso/FullSystem/CoarseInitializer.cpp:85-281) on the
// resident point sets of capi_init_resident.hip.  This unit fills the problem records, keeps the context's LM record and enqueues; the loop itself is k_init_lm
// (init_lm_kernels.hpp).
#include <vector>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <algorithm>
#include "../../include/dmvio_hip_init_lm.h"
#include "init_handle.h"
#include "init_resident_state.h"
#include "init_lm_kernels.hpp"

using namespace dmv;

static_assert(INIT_LM_TRACE_D == DMVIO_HIP_INIT_LM_TRACE_D && INIT_LM_TRACE_F == DMVIO_HIP_INIT_LM_TRACE_F, "the header states the trace's record");
enum { LM_TRACE_MAX = DMV_MAX_LEVELS * (INIT_LM_MAX_ITER + 1) };

// One slab per context: [problem records | the LM record | per-problem results | trace].  An upload covers the records, or the records and the LM record; the download
// starts at the LM record.  `sent`: the records as the device holds them — a call whose records equal them uploads nothing.
struct DmvInitLmCtx {
  DmvSlab slab;
  DmvWork work;
  size_t o_state = 0, o_outs = 0, o_trace = 0, total = 0;
  std::vector<char> sent;
  bool holds_state = false;
  size_t lds_limit = 0, lds_static = 0;
  InitLmControlIo* d_ctl = nullptr;
};

void dmvInitLmRelease(dmvio_hip_ctx* c) {
  if (!c->init_lm) return;
  c->init_lm->slab.release();
  if (c->init_lm->d_ctl) hipFree(c->init_lm->d_ctl);
  delete c->init_lm;
  c->init_lm = nullptr;
}

// the context's LM state, made on first use (under the context's lock)
static int lmCtx(dmvio_hip_ctx* c, DmvInitLmCtx** out) {
  if (!c->init_lm) {
    int lim = 0;
    HIPCHK(hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
    if (lim <= 0) return failmsg("initializer LM loop: the device reports no LDS per workgroup");
    hipFuncAttributes fa;
    HIPCHK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_init_lm)));
    if (fa.sharedSizeBytes >= (size_t)lim) return failmsg("initializer LM loop: the kernel's own LDS exceeds what the device allows a workgroup");
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_init_lm), hipFuncAttributeMaxDynamicSharedMemorySize, lim - (int)fa.sharedSizeBytes));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_init_lm_opt_reg), hipFuncAttributeMaxDynamicSharedMemorySize, lim));
    DmvInitLmCtx* L = new DmvInitLmCtx();
    DmvCursor cur;
    cur.take<InitLmProb>(DMV_MAX_LEVELS);
    L->o_state = cur.take<InitLmState>(1); L->o_outs = cur.take<InitLmOut>(DMV_MAX_LEVELS); L->o_trace = cur.take<InitLmTraceRec>(LM_TRACE_MAX);
    L->total = cur.bytes();
    L->slab.work = &L->work;
    if (int r = L->slab.create(L->total)) { L->slab.release(); delete L; return r; }
    L->lds_limit = (size_t)lim; L->lds_static = fa.sharedSizeBytes;
    c->init_lm = L;
  }
  *out = c->init_lm;
  return 0;
}

struct LmLevel { dmvio_hip_initializer* m; int lvl, max_iterations, is_top_level; const double* Ki9; const float* K4; };
struct LmCommon {
  int first_slot, new_slot, fix_affine;
  float alphaW, alphaK, regWeight, couplingWeight;
  double priorY, priorX;
  const float* wM8;
};

// every refusal of a call, in the header's order; P levels in execution order (the top level first)
// first_outside (may be NULL): for a level whose loop revives no point — a lone track_level that is not the top level — a point outside the margin is no refusal here;
// its index comes back and the caller counts the GOOD points outside on the device, as dmvio_hip_initializer_resident_calc does.  Everywhere else (the top level's
// resetPoints and a frame's propagateDown turn bad points into good ones inside the call) any point outside refuses.
static int lmCheck(const char* who, dmvio_hip_ctx* c, DmvInitLmCtx* L, const LmLevel* lv, int P, const LmCommon& K, const double* state_in10, int trace_capacity,
                   const double* trace_d, const float* trace_f, const int* trace_records, int* first_outside) {
  if (first_outside) *first_outside = -1;
  char msg[320];
  auto no = [&](const char* what) { snprintf(msg, sizeof(msg), "%s: %s", who, what); return failmsg(msg); };
  if (!K.wM8) return no("null wM8");
  if (K.first_slot < 0 || K.first_slot >= c->n_slots || K.new_slot < 0 || K.new_slot >= c->n_slots) return no("slot out of range");
  int tests = 0;
  for (int p = 0; p < P; p++) {
    const LmLevel& v = lv[p];
    if (!v.Ki9 || !v.K4) return no("null argument");
    if (!v.m->resident || !v.m->resident->live) { snprintf(msg, sizeof(msg), "%s: the handle of level %d has no resident point set (dmvio_hip_initializer_set_resident)", who, v.lvl); return failmsg(msg); }
    if (v.lvl < 0 || v.lvl >= c->levels) return no("level out of range");
    if (v.max_iterations < 0 || v.max_iterations > INIT_LM_MAX_ITER) { snprintf(msg, sizeof(msg), "%s: max_iterations = %d outside [0, %d]", who, v.max_iterations, (int)INIT_LM_MAX_ITER); return failmsg(msg); }
    tests += v.max_iterations + 1;
    const DmvInitResident* R = v.m->resident;
    if (p > 0) {   // lv[p - 1] is the level above
      const DmvInitResident* U = lv[p - 1].m->resident;
      if (!R->has_parent) { snprintf(msg, sizeof(msg), "%s: level %d was set without a parent table", who, v.lvl); return failmsg(msg); }
      if (R->max_parent >= U->n) { snprintf(msg, sizeof(msg), "%s: level %d names parent %d, level %d has %d points", who, v.lvl, R->max_parent, lv[p - 1].lvl, U->n); return failmsg(msg); }
    }
    const float *hu = R->st.host<float>(R->o_u), *hv = R->st.host<float>(R->o_v);
    const float umax = (float)(c->wl[v.lvl] - 3), vmax = (float)(c->hl[v.lvl] - 3);
    for (int i = 0; i < R->n; i++)
      if (!(hu[i] >= 2.0f && hu[i] < umax && hv[i] >= 2.0f && hv[i] < vmax)) {
        if (first_outside && !v.is_top_level) { *first_outside = i; break; }
        snprintf(msg, sizeof(msg), "%s: point %d of level %d at (%g, %g) outside [2, %d) x [2, %d): the loop may revive and then evaluate any point of the level", who, i, v.lvl,
                 (double)hu[i], (double)hv[i], c->wl[v.lvl] - 3, c->hl[v.lvl] - 3);
        return failmsg(msg);
      }
    if (L->lds_static + resSweepLds(R->n) > L->lds_limit) {
      snprintf(msg, sizeof(msg), "%s: the loop of level %d with n = %d points needs %zu bytes of LDS (%zu of its own and 5 n for the ordered sweeps), the device allows a workgroup %zu", who,
               v.lvl, R->n, L->lds_static + resSweepLds(R->n), L->lds_static, L->lds_limit);
      return failmsg(msg);
    }
  }
  if (!state_in10 && !L->holds_state) return no("state_in10 is NULL and the context's record holds no state yet");
  if (trace_d || trace_f) {
    if (!trace_d || !trace_f || !trace_records) return no("a trace needs trace_d, trace_f and trace_records");
    if (trace_capacity < tests) { snprintf(msg, sizeof(msg), "%s: trace_capacity = %d, the call can make %d accept tests", who, trace_capacity, tests); return failmsg(msg); }
  }
  return 0;
}

static void lmFillProb(InitLmProb& Q, dmvio_hip_ctx* c, const LmLevel& v, const LmCommon& K, int p, int trace_base) {
  const DmvInitResident* R = v.m->resident;
  memset(&Q, 0, sizeof(Q));   // (padding too: the records are compared as bytes)
  Q.Iref = c->frames.levelPtr(K.first_slot, v.lvl); Q.Inew = c->frames.levelPtr(K.new_slot, v.lvl);
  Q.u = R->f(R->o_u); Q.v = R->f(R->o_v); Q.outlierTH = R->f(R->o_oth);
  Q.idepth = R->f(R->o_idepth); Q.idepth_new = R->f(R->o_idn); Q.iR = R->f(R->o_iR); Q.energy = R->f(R->o_energy); Q.energy_new = R->f(R->o_en_new);
  Q.maxstep = R->f(R->o_maxstep); Q.lastHessian = R->f(R->o_lh); Q.lastHessian_new = R->f(R->o_lh_new); Q.jb[0] = R->f(R->o_jb[0]); Q.jb[1] = R->f(R->o_jb[1]);
  Q.isGood = R->b(R->o_good); Q.isGood_new = R->b(R->o_good_new);
  Q.level_begin = R->i(R->o_lbegin); Q.order = R->i(R->o_order); Q.neighbours = R->i(R->o_nb);
  Q.partials = R->io.dev<float>(0) + RES_OUT_FLOATS; Q.ecpartials = Q.partials + (size_t)INIT_EVAL_MAX_BLOCKS * IN_PART;
  for (int k = 0; k < 9; k++) Q.Ki9[k] = v.Ki9[k];
  Q.priorY = K.priorY; Q.priorX = K.priorX;
  for (int k = 0; k < 4; k++) Q.fxfycxcy[k] = v.K4[k];
  for (int k = 0; k < 8; k++) Q.wM8[k] = K.wM8[k];
  Q.alphaW = K.alphaW; Q.alphaK = K.alphaK; Q.regWeight = K.regWeight; Q.couplingWeight = K.couplingWeight;
  Q.n = R->n; Q.G = initEvalGrid(R->n); Q.sweep_levels = R->levels; Q.cur = R->cur; Q.wl = c->wl[v.lvl]; Q.hl = c->hl[v.lvl]; Q.lvl = v.lvl;
  Q.is_top_level = v.is_top_level; Q.fix_affine = K.fix_affine; Q.max_iterations = v.max_iterations; Q.out_index = p; Q.trace_base = trace_base;
}

// the checked call: records, the state, the launches, and — with state_out10 — the download, the wait and the delivery.  frame: the reset, propagateDown / Up around the loops.
static int lmRun(dmvio_hip_ctx* c, DmvInitLmCtx* L, const LmLevel* lv, int P, const LmCommon& K, bool frame, const double* state_in10, double* state_out10, float* res3,
                 int* iterations, double* trace_d, float* trace_f, int* trace_records) {
  hipStream_t s = c->stream;
  for (int p = 0; p < P; p++)
    if (lv[p].lvl == 0) { if (int r = dmv_ensure_row_major_locked(c, K.first_slot)) return r; if (int r = dmv_ensure_row_major_locked(c, K.new_slot)) return r; }   // (not counted, as in the host-driven calls)
  L->work.clear();
  std::vector<char> rec(sizeof(InitLmProb) * (size_t)DMV_MAX_LEVELS, 0);
  InitLmProb* Q = reinterpret_cast<InitLmProb*>(rec.data());
  int trace_base = 0;
  for (int p = 0; p < P; p++) { lmFillProb(Q[p], c, lv[p], K, p, trace_base); trace_base += lv[p].max_iterations + 1; }
  const bool new_records = L->sent != rec;
  if (new_records || state_in10) {
    if (int r = L->slab.begin(s)) return r;
    memcpy(L->slab.host<char>(0), rec.data(), rec.size());
    size_t bytes = L->o_state;
    if (state_in10) {
      InitLmState* S = L->slab.host<InitLmState>(L->o_state);
      memset(S, 0, sizeof(*S));
      for (int k = 0; k < 7; k++) S->pose7[k] = state_in10[k];
      S->aff[0] = state_in10[7]; S->aff[1] = state_in10[8]; S->snapped = state_in10[9] != 0.0;
      bytes = L->o_state + sizeof(InitLmState);
    }
    L->sent.clear();
    if (int r = L->slab.upload(s, bytes)) return r;
    L->sent = rec;
    if (state_in10) L->holds_state = true;
  }
  const InitLmProb* d_probs = L->slab.dev<const InitLmProb>(0);
  InitLmState* d_state = L->slab.dev<InitLmState>(L->o_state);
  InitLmOut* d_outs = L->slab.dev<InitLmOut>(L->o_outs);
  InitLmTraceRec* d_trace = trace_d ? L->slab.dev<InitLmTraceRec>(L->o_trace) : nullptr;
  auto optReg = [&](int p) {   // behind a propagate call: where the record says snapped
    const int n = lv[p].m->resident->n;
    if (n == 0) return;
    hipLaunchKernelGGL(k_init_lm_opt_reg, dim3(1), dim3(64), resSweepLds(n), s, d_probs + p, d_state);
    L->work.launches++;
  };
  if (frame) {
    int most = 0;
    for (int p = 0; p < P; p++) most = std::max(most, lv[p].m->resident->n);
    hipLaunchKernelGGL(k_init_lm_frame_begin, dim3((unsigned)std::max(1, (most + 255) / 256), (unsigned)P), dim3(256), 0, s, d_probs, d_state);
    L->work.launches++;
  }
  for (int p = 0; p < P; p++) {
    DmvInitResident* R = lv[p].m->resident;
    if (frame && p > 0 && R->n) {   // propagateDown from the level above (:749-777)
      DmvInitResident* U = lv[p - 1].m->resident;
      hipLaunchKernelGGL(k_init_propagate_down, dim3((unsigned)((R->n + 255) / 256)), dim3(256), 0, s, R->n, R->i(R->o_parent), U->b(U->o_good), U->f(U->o_iR), U->f(U->o_lh),
                         R->b(R->o_good), R->f(R->o_iR), R->f(R->o_idepth), R->f(R->o_idn), R->f(R->o_lh));
      L->work.launches++;
      optReg(p);
    }
    hipLaunchKernelGGL(k_init_lm, dim3(1), dim3(256), resSweepLds(R->n), s, d_probs + p, d_state, d_outs, d_trace);
    L->work.launches++;
  }
  if (frame)
    for (int p = P - 1; p > 0; p--) {   // propagateUp from level lv[p] into lv[p - 1], the lowest pair first (:262-263)
      DmvInitResident *Lo = lv[p].m->resident, *R = lv[p - 1].m->resident;
      if (!R->n) continue;
      hipLaunchKernelGGL(k_init_propagate_up, dim3((unsigned)((R->n + 255) / 256)), dim3(256), 0, s, R->n, Lo->n_listed, Lo->i(Lo->o_cbegin), Lo->i(Lo->o_children),
                         Lo->b(Lo->o_good), Lo->f(Lo->o_iR), Lo->f(Lo->o_lh), R->f(R->o_iR), R->f(R->o_idepth), R->b(R->o_good));
      L->work.launches++;
      optReg(p - 1);
    }
  HIPCHK(hipGetLastError());
  if (!state_out10) return 0;
  const size_t down = (trace_d ? L->o_trace + sizeof(InitLmTraceRec) * (size_t)trace_base : L->o_trace) - L->o_state;
  if (int r = L->slab.download(s, L->o_state, down)) return r;
  if (int r = L->slab.wait(s)) return r;
  for (int p = 0; p < P; p++) lv[p].m->resident->st.settled();
  const InitLmState* S = L->slab.host<InitLmState>(L->o_state);
  for (int k = 0; k < 7; k++) state_out10[k] = S->pose7[k];
  state_out10[7] = S->aff[0]; state_out10[8] = S->aff[1]; state_out10[9] = S->snapped ? 1.0 : 0.0;
  const InitLmOut* O = L->slab.host<InitLmOut>(L->o_outs);
  int written = 0;
  for (int p = 0; p < P; p++) {
    const int at = frame ? lv[p].lvl : 0;   // the frame call's arrays are indexed by level
    if (res3) for (int k = 0; k < 3; k++) res3[3 * at + k] = O[p].res3[k];
    if (iterations) iterations[at] = O[p].iterations;
    if (trace_d) {
      const InitLmTraceRec* T = L->slab.host<InitLmTraceRec>(L->o_trace) + Q[p].trace_base;
      for (int k = 0; k < O[p].tests; k++, written++) {
        memcpy(trace_d + (size_t)written * INIT_LM_TRACE_D, T[k].d, sizeof(T[k].d));
        memcpy(trace_f + (size_t)written * INIT_LM_TRACE_F, T[k].f, sizeof(T[k].f));
      }
    }
  }
  if (trace_d) *trace_records = written;
  return S->snapped ? 1 : 0;
}

extern "C" {

int dmvio_hip_initializer_lm_control_host(const float* H64, const float* b8, const float* Hsc64, const float* bsc8, float lambda, int wh, const float* wM8, int fix_affine,
                                          const double* refToNew7, const double* aff_ab, float* inc8, double* incNorm, double* refToNew7_new, double* aff_ab_new) {
  if (!H64 || !b8 || !Hsc64 || !bsc8 || !wM8 || !refToNew7 || !aff_ab || !inc8 || !incNorm || !refToNew7_new || !aff_ab_new) return failmsg("initializer_lm_control_host: null argument");
  if (wh <= 0) return failmsg("initializer_lm_control_host: wh is not positive");
  InitLmWs ws;
  float inc[8];
  double norm, pose[7], aff[2];
  initLmControl(H64, b8, Hsc64, bsc8, lambda, wh, wM8, fix_affine, refToNew7, aff_ab, ws, inc, &norm, pose, aff);
  memcpy(inc8, inc, sizeof(inc)); *incNorm = norm; memcpy(refToNew7_new, pose, sizeof(pose)); memcpy(aff_ab_new, aff, sizeof(aff));
  return 0;
}

int dmvio_hip_initializer_debug_lm_control(dmvio_hip_ctx* c, const float* H64, const float* b8, const float* Hsc64, const float* bsc8, float lambda, int wh, const float* wM8,
                                           int fix_affine, const double* refToNew7, const double* aff_ab, float* inc8, double* incNorm, double* refToNew7_new,
                                           double* aff_ab_new) {
  if (!c) return failmsg("initializer_debug_lm_control: null context");
  if (!H64 || !b8 || !Hsc64 || !bsc8 || !wM8 || !refToNew7 || !aff_ab || !inc8 || !incNorm || !refToNew7_new || !aff_ab_new) return failmsg("initializer_debug_lm_control: null argument");
  if (wh <= 0) return failmsg("initializer_debug_lm_control: wh is not positive");
  HIPCHK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  DmvInitLmCtx* L;
  if (int r = lmCtx(c, &L)) return r;
  if (!L->d_ctl) HIPCHK(hipMalloc((void**)&L->d_ctl, sizeof(InitLmControlIo)));
  InitLmControlIo io;
  memset(&io, 0, sizeof(io));
  memcpy(io.H, H64, sizeof(io.H)); memcpy(io.b, b8, sizeof(io.b)); memcpy(io.Hsc, Hsc64, sizeof(io.Hsc)); memcpy(io.bsc, bsc8, sizeof(io.bsc)); memcpy(io.wM, wM8, sizeof(io.wM));
  io.lambda = lambda; io.wh = wh; io.fix_affine = fix_affine;
  memcpy(io.pose7, refToNew7, sizeof(io.pose7)); memcpy(io.aff, aff_ab, sizeof(io.aff));
  hipStream_t s = c->stream;
  HIPCHK(c->bounce.h2d(L->d_ctl, &io, sizeof(io), s));
  hipLaunchKernelGGL(k_init_debug_lm_control, dim3(1), dim3(64), 0, s, L->d_ctl);
  HIPCHK(hipGetLastError());
  InitLmControlIo out;
  HIPCHK(c->bounce.d2h(&out, L->d_ctl, sizeof(out), s));
  HIPCHK(c->bounce.finish(s));
  memcpy(inc8, out.inc, sizeof(out.inc)); *incNorm = out.incNorm; memcpy(refToNew7_new, out.pose7_new, sizeof(out.pose7_new)); memcpy(aff_ab_new, out.aff_new, sizeof(out.aff_new));
  return 0;
}

int dmvio_hip_initializer_resident_track_level(dmvio_hip_initializer* m, int lvl, int first_slot, int new_slot, const double* Ki9, const float* fxfycxcy_lvl, float alphaW,
                                               float alphaK, float regWeight, float couplingWeight, double priorY, double priorX, const float* wM8, int fix_affine,
                                               int max_iterations, int is_top_level, const double* state_in10, double* state_out10, float* res3, int* iterations,
                                               int trace_capacity, double* trace_d, float* trace_f, int* trace_records) {
  static const char* who = "initializer_resident_track_level";
  if (!m) return failmsg("initializer_resident_track_level: null initializer handle");
  HIPCHK(hipSetDevice(m->ctx->device));
  dmvio_hip_ctx* c = m->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  DmvInitLmCtx* L;
  if (int r = lmCtx(c, &L)) return r;
  const LmLevel lv = {m, lvl, max_iterations, is_top_level != 0, Ki9, fxfycxcy_lvl};
  const LmCommon K = {first_slot, new_slot, fix_affine != 0, alphaW, alphaK, regWeight, couplingWeight, priorY, priorX, wM8};
  int first = -1;
  if (int r = lmCheck(who, c, L, &lv, 1, K, state_in10, trace_capacity, trace_d, trace_f, trace_records, &first)) return r;
  if (first >= 0) {   // the range condition of resident_calc: the good points outside, counted on the device in a download and a wait of their own, before the loop is enqueued
    DmvInitResident* R = m->resident;
    hipStream_t s = c->stream;
    const float umax = (float)(c->wl[lvl] - 3), vmax = (float)(c->hl[lvl] - 3);
    int* d_count = R->io.dev<int>(sizeof(float) * RES_COUNT);
    HIPCHK(hipMemsetAsync(d_count, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_init_count_outside, dim3((unsigned)((R->n + 255) / 256)), dim3(256), 0, s, R->n, R->b(R->o_good), R->f(R->o_u), R->f(R->o_v), umax, vmax, d_count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(R->io.host<int>(sizeof(float) * RES_COUNT), d_count, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int outside = *R->io.host<int>(sizeof(float) * RES_COUNT);
    if (outside) {
      char msg[256];
      snprintf(msg, sizeof(msg), "%s: %d good point(s) outside [2, %d) x [2, %d) of level %d (the first point outside, good or not, is %d)", who, outside, c->wl[lvl] - 3, c->hl[lvl] - 3, lvl, first);
      return failmsg(msg);
    }
  }
  const int r = lmRun(c, L, &lv, 1, K, false, state_in10, state_out10, res3, iterations, trace_d, trace_f, trace_records);
  return r < 0 ? r : 0;
}

int dmvio_hip_initializer_resident_track_frame(dmvio_hip_initializer* const* levels, int n_levels, int first_slot, int new_slot, const double* Ki9_levels,
                                               const float* fxfycxcy_levels, float alphaW, float alphaK, float regWeight, float couplingWeight, double priorY, double priorX,
                                               const float* wM8, int fix_affine, const int* max_iterations, const double* state_in10, double* state_out10, float* res3_levels,
                                               int* iterations_levels, int trace_capacity, double* trace_d, float* trace_f, int* trace_records) {
  static const char* who = "initializer_resident_track_frame";
  if (!levels || n_levels < 1 || !levels[0]) return failmsg("initializer_resident_track_frame: null handle array, null handle or n_levels < 1");
  dmvio_hip_ctx* c = levels[0]->ctx;
  char msg[200];
  if (n_levels > c->levels) { snprintf(msg, sizeof(msg), "%s: n_levels = %d outside [1, %d], the context's levels", who, n_levels, c->levels); return failmsg(msg); }
  for (int k = 0; k < n_levels; k++) {
    if (!levels[k]) { snprintf(msg, sizeof(msg), "%s: null initializer handle of level %d", who, k); return failmsg(msg); }
    if (levels[k]->ctx != c) { snprintf(msg, sizeof(msg), "%s: the handle of level %d belongs to another context", who, k); return failmsg(msg); }
    for (int j = 0; j < k; j++)
      if (levels[j] == levels[k]) { snprintf(msg, sizeof(msg), "%s: the handle of level %d named again as level %d", who, j, k); return failmsg(msg); }
  }
  if (!Ki9_levels || !fxfycxcy_levels || !max_iterations) return failmsg("initializer_resident_track_frame: null argument");
  HIPCHK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  DmvInitLmCtx* L;
  if (int r = lmCtx(c, &L)) return r;
  LmLevel lv[DMV_MAX_LEVELS];
  for (int p = 0; p < n_levels; p++) {   // execution order: the top level first
    const int l = n_levels - 1 - p;
    lv[p] = {levels[l], l, max_iterations[l], p == 0, Ki9_levels + 9 * (size_t)l, fxfycxcy_levels + 4 * (size_t)l};
  }
  const LmCommon K = {first_slot, new_slot, fix_affine != 0, alphaW, alphaK, regWeight, couplingWeight, priorY, priorX, wM8};
  if (int r = lmCheck(who, c, L, lv, n_levels, K, state_in10, trace_capacity, trace_d, trace_f, trace_records, nullptr)) return r;
  return lmRun(c, L, lv, n_levels, K, true, state_in10, state_out10, res3_levels, iterations_levels, trace_d, trace_f, trace_records);
}

int dmvio_hip_initializer_lm_last_work(dmvio_hip_ctx* c, int* launches, int* uploads, int* downloads, int* waits) {
  if (!c) return failmsg("initializer_lm_last_work: null context");
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->init_lm) c->init_lm->work.report(launches, uploads, downloads, waits);
  else DmvWork().report(launches, uploads, downloads, waits);
  return 0;
}

}  // extern "C"
