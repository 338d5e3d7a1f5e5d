// C ABI of the initializer's LM loop on the device (include/dmvio_hip_init_lm.h): CoarseInitializer::trackFrame (src/dso/FullSystem/CoarseInitializer.cpp:85-281) on the
// resident point sets of capi_init_resident.hip.  This unit keeps the context's LM record and enqueues; the loop itself is k_init_lm (init_lm_kernels.hpp), the
// propagation around it and the outside count are the resident unit's launches (init_resident_state.h), and what a call checks, sends and hands back is shared with the
// batched call (init_lm_host.hpp).
#include <vector>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <algorithm>
#include "../../include/dmvio_hip_init_lm.h"
#include "init_lm_host.hpp"   // the handle, the resident state, the kernels; a call's levels, lmCheck, lmFillProb, lmSend and lmDeliver

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
    size_t own = 0, own_reg = 0;
    HIPCHK(initLdsAllow(c->device, &lim, reinterpret_cast<const void*>(&k_init_lm), &own));
    if (lim <= 0) return failmsg("initializer LM loop: the device reports no LDS per workgroup");
    if (own >= (size_t)lim) return failmsg("initializer LM loop: the kernel's own LDS exceeds what the device allows a workgroup");
    HIPCHK(initLdsAllow(c->device, &lim, reinterpret_cast<const void*>(&k_init_lm_opt_reg), &own_reg));
    DmvInitLmCtx* L = new DmvInitLmCtx();
    DmvCursor cur;
    cur.take<InitLmProb>(DMV_MAX_LEVELS);
    L->o_state = cur.take<InitLmState>(1); L->o_outs = cur.take<InitLmOut>(DMV_MAX_LEVELS); L->o_trace = cur.take<InitLmTraceRec>(LM_TRACE_MAX);
    L->total = cur.bytes();
    L->slab.work = &L->work;
    if (int r = L->slab.create(L->total)) { L->slab.release(); delete L; return r; }
    L->lds_limit = (size_t)lim; L->lds_static = own;
    c->init_lm = L;
  }
  *out = c->init_lm;
  return 0;
}

// what lmCheck (init_lm_host.hpp) reads of this unit's kernel and record
static LmLimits lmLimits(const DmvInitLmCtx* L) { return {L->lds_static, L->lds_limit, L->holds_state, "the context's record"}; }

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
  if (int r = lmSend(L->slab, L->sent, rec, state_in10 != nullptr, state_in10 ? L->o_state + sizeof(InitLmState) : L->o_state, s,
                     [&] { lmStateFrom10(L->slab.host<InitLmState>(L->o_state), state_in10); })) return r;
  if (state_in10) L->holds_state = true;
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
    if (frame && p > 0) {   // propagateDown from the level above (:749-777)
      if (int r = resPropagateDown(R, lv[p - 1].m->resident, s, &L->work)) return r;
      optReg(p);
    }
    hipLaunchKernelGGL(k_init_lm, dim3(1), dim3(256), resSweepLds(R->n), s, d_probs + p, d_state, d_outs, d_trace);
    L->work.launches++;
  }
  if (frame)
    for (int p = P - 1; p > 0; p--) {   // propagateUp from level lv[p] into lv[p - 1], the lowest pair first (:262-263)
      if (int r = resPropagateUp(lv[p - 1].m->resident, lv[p].m->resident, s, &L->work)) return r;
      optReg(p - 1);
    }
  HIPCHK(hipGetLastError());
  if (!state_out10) return 0;
  const size_t down = (trace_d ? L->o_trace + sizeof(InitLmTraceRec) * (size_t)trace_base : L->o_trace) - L->o_state;
  if (int r = L->slab.download(s, L->o_state, down)) return r;
  if (int r = L->slab.wait(s)) return r;
  const InitLmState* S = L->slab.host<InitLmState>(L->o_state);
  lmStateTo10(S, state_out10);
  lmDeliver(lv, P, Q, L->slab.host<InitLmOut>(L->o_outs), L->slab.host<InitLmTraceRec>(L->o_trace), frame, res3, iterations, trace_d, trace_f, trace_records);
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
  if (int r = lmCheck(who, c, lmLimits(L), &lv, 1, K, state_in10, trace_capacity, trace_d, trace_f, trace_records, &first)) return r;
  if (first >= 0) {   // the range condition of resident_calc: the good points outside, counted on the device in a download and a wait of their own, before the loop is enqueued
    int outside = 0;
    if (int r = resCountOutside(m->resident, c->wl[lvl], c->hl[lvl], c->stream, nullptr, &outside)) return r;   // (counted nowhere: last_work reports the loop's call)
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
  lmFrameLevels(lv, levels, n_levels, max_iterations, Ki9_levels, fxfycxcy_levels);
  const LmCommon K = {first_slot, new_slot, fix_affine != 0, alphaW, alphaK, regWeight, couplingWeight, priorY, priorX, wM8};
  if (int r = lmCheck(who, c, lmLimits(L), lv, n_levels, K, state_in10, trace_capacity, trace_d, trace_f, trace_records, nullptr)) return r;
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
