// What the two host units of the initializer's LM loop share (capi_init_lm.hip: one frame or one level per call; capi_init_lm_batch.hip: the frames of W windows per call): a
// call's levels and common arguments (lmFrameLevels), every per-window refusal (lmCheck), the problem record of one level (lmFillProb), the upload of the records where
// the device does not hold them already (lmSend) and the delivery of a frame's results (lmDeliver).  One copy, so that a batched window is refused by the rules of its
// single call, runs on the record its single call would have sent and hands back what that call would have.
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>
#include "init_handle.h"
#include "init_resident_state.h"
#include "init_lm_kernels.hpp"

struct LmLevel { dmvio_hip_initializer* m; int lvl, max_iterations, is_top_level; const double* Ki9; const float* K4; };
struct LmCommon {
  int first_slot, new_slot, fix_affine;
  float alphaW, alphaK, regWeight, couplingWeight;
  double priorY, priorX;
  const float* wM8;
};
// the levels of a frame in execution order, the top level first, from the C ABI's arrays indexed by level; returns the accept tests the frame can make
static inline int lmFrameLevels(LmLevel* lv, dmvio_hip_initializer* const* levels, int n_levels, const int* max_iterations, const double* Ki9_levels, const float* fxfycxcy_levels) {
  int tests = 0;
  for (int p = 0; p < n_levels; p++) {
    const int l = n_levels - 1 - p;
    lv[p] = {levels[l], l, max_iterations[l], p == 0, Ki9_levels + 9 * (size_t)l, fxfycxcy_levels + 4 * (size_t)l};
    tests += max_iterations[l] + 1;
  }
  return tests;
}
// what of the unit's kernel and record a check reads: the kernel's own LDS and the device's limit, whether the record the call would continue from holds a state, and that
// record's name for the refusal
struct LmLimits { size_t lds_static, lds_limit; bool holds_state; const char* record; };

// every refusal of a call, in the header's order; P levels in execution order (the top level first)
// first_outside (may be NULL): for a level whose loop revives no point — a lone track_level that is not the top level — a point outside the margin is no refusal here;
// its index comes back and the caller counts the GOOD points outside on the device, as dmvio_hip_initializer_resident_calc does.  Everywhere else (the top level's
// resetPoints and a frame's propagateDown turn bad points into good ones inside the call) any point outside refuses.
static inline int lmCheck(const char* who, dmvio_hip_ctx* c, const LmLimits& L, const LmLevel* lv, int P, const LmCommon& K, const double* state_in10, int trace_capacity,
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
    if (v.max_iterations < 0 || v.max_iterations > dmv::INIT_LM_MAX_ITER) { snprintf(msg, sizeof(msg), "%s: max_iterations = %d outside [0, %d]", who, v.max_iterations, (int)dmv::INIT_LM_MAX_ITER); return failmsg(msg); }
    tests += v.max_iterations + 1;
    const DmvInitResident* R = v.m->resident;
    if (p > 0) {   // lv[p - 1] is the level above
      const DmvInitResident* U = lv[p - 1].m->resident;
      if (!R->has_parent) { snprintf(msg, sizeof(msg), "%s: level %d was set without a parent table", who, v.lvl); return failmsg(msg); }
      if (R->max_parent >= U->n) { snprintf(msg, sizeof(msg), "%s: level %d names parent %d, level %d has %d points", who, v.lvl, R->max_parent, lv[p - 1].lvl, U->n); return failmsg(msg); }
    }
    const int i = resFirstOutside(R, c->wl[v.lvl], c->hl[v.lvl]);
    if (i >= 0 && first_outside && !v.is_top_level) *first_outside = i;
    else if (i >= 0) {
      snprintf(msg, sizeof(msg), "%s: point %d of level %d at (%g, %g) outside [2, %d) x [2, %d): the loop may revive and then evaluate any point of the level", who, i, v.lvl,
               (double)R->st.host<float>(R->o_u)[i], (double)R->st.host<float>(R->o_v)[i], c->wl[v.lvl] - 3, c->hl[v.lvl] - 3);
      return failmsg(msg);
    }
    if (L.lds_static + resSweepLds(R->n) > L.lds_limit) {
      snprintf(msg, sizeof(msg), "%s: the loop of level %d with n = %d points needs %zu bytes of LDS (%zu of its own and 5 n for the ordered sweeps), the device allows a workgroup %zu", who,
               v.lvl, R->n, L.lds_static + resSweepLds(R->n), L.lds_static, L.lds_limit);
      return failmsg(msg);
    }
  }
  if (!state_in10 && !L.holds_state) { snprintf(msg, sizeof(msg), "%s: state_in10 is NULL and %s holds no state yet", who, L.record); return failmsg(msg); }
  if (trace_d || trace_f) {
    if (!trace_d || !trace_f || !trace_records) return no("a trace needs trace_d, trace_f and trace_records");
    if (trace_capacity < tests) { snprintf(msg, sizeof(msg), "%s: trace_capacity = %d, the call can make %d accept tests", who, trace_capacity, tests); return failmsg(msg); }
  }
  return 0;
}

// the record of level v; out_index: where the level's InitLmOut goes, trace_base: its first trace record
static inline void lmFillProb(dmv::InitLmProb& Q, dmvio_hip_ctx* c, const LmLevel& v, const LmCommon& K, int out_index, int trace_base) {
  const DmvInitResident* R = v.m->resident;
  memset(&Q, 0, sizeof(Q));   // (padding too: the records are compared as bytes)
  Q.Iref = c->frames.levelPtr(K.first_slot, v.lvl); Q.Inew = c->frames.levelPtr(K.new_slot, v.lvl);
  Q.u = R->f(R->o_u); Q.v = R->f(R->o_v); Q.outlierTH = R->f(R->o_oth);
  Q.idepth = R->f(R->o_idepth); Q.idepth_new = R->f(R->o_idn); Q.iR = R->f(R->o_iR); Q.energy = R->f(R->o_energy); Q.energy_new = R->f(R->o_en_new);
  Q.maxstep = R->f(R->o_maxstep); Q.lastHessian = R->f(R->o_lh); Q.lastHessian_new = R->f(R->o_lh_new); Q.jb[0] = R->f(R->o_jb[0]); Q.jb[1] = R->f(R->o_jb[1]);
  Q.isGood = R->b(R->o_good); Q.isGood_new = R->b(R->o_good_new);
  Q.level_begin = R->i(R->o_lbegin); Q.order = R->i(R->o_order); Q.neighbours = R->i(R->o_nb);
  Q.partials = R->io.dev<float>(0) + RES_OUT_FLOATS; Q.ecpartials = Q.partials + (size_t)INIT_MAX_BLOCKS * dmv::IN_PART;
  for (int k = 0; k < 9; k++) Q.Ki9[k] = v.Ki9[k];
  Q.priorY = K.priorY; Q.priorX = K.priorX;
  for (int k = 0; k < 4; k++) Q.fxfycxcy[k] = v.K4[k];
  for (int k = 0; k < 8; k++) Q.wM8[k] = K.wM8[k];
  Q.alphaW = K.alphaW; Q.alphaK = K.alphaK; Q.regWeight = K.regWeight; Q.couplingWeight = K.couplingWeight;
  Q.n = R->n; Q.G = initGrid(R->n); Q.sweep_levels = R->levels; Q.cur = R->cur; Q.wl = c->wl[v.lvl]; Q.hl = c->hl[v.lvl]; Q.lvl = v.lvl;
  Q.is_top_level = v.is_top_level; Q.fix_affine = K.fix_affine; Q.max_iterations = v.max_iterations; Q.out_index = out_index; Q.trace_base = trace_base;
}
// the state record from the ten doubles of the C ABI, and back
static inline void lmStateFrom10(dmv::InitLmState* S, const double* state10) {
  memset(S, 0, sizeof(*S));
  for (int k = 0; k < 7; k++) S->pose7[k] = state10[k];
  S->aff[0] = state10[7]; S->aff[1] = state10[8]; S->snapped = state10[9] != 0.0;
}
static inline void lmStateTo10(const dmv::InitLmState* S, double* state10) {
  for (int k = 0; k < 7; k++) state10[k] = S->pose7[k];
  state10[7] = S->aff[0]; state10[8] = S->aff[1]; state10[9] = S->snapped ? 1.0 : 0.0;
}

// The records of a call, sent unless the device holds them already.  `sent`: the records as the head of the slab on the device holds them; a call whose records equal
// them and that brings nothing else (`more`) uploads nothing.  Otherwise the pinned side is taken, the records go to its head, fill() writes what else goes up behind
// them, and the first `bytes` are uploaded.
template <class FILL>
static inline int lmSend(DmvSlab& slab, std::vector<char>& sent, const std::vector<char>& rec, bool more, size_t bytes, hipStream_t s, const FILL& fill) {
  if (!more && sent == rec) return 0;
  if (int r = slab.begin(s)) return r;
  memcpy(slab.host<char>(0), rec.data(), rec.size());
  if (more) fill();
  sent.clear();   // (a failed upload leaves the device's records unknown)
  if (int r = slab.upload(s, bytes)) return r;
  sent = rec;
  return 0;
}
// Behind the call's wait: the results of a frame's P levels into the caller's arrays (each may be NULL; trace_records with trace_d).  Q, O: the frame's problem records and
// their results; T: the call's trace records, which Q's trace_base indexes.  by_level: res3 and iterations are indexed by level (a frame call), else the one level's go first.
static inline void lmDeliver(const LmLevel* lv, int P, const dmv::InitLmProb* Q, const dmv::InitLmOut* O, const dmv::InitLmTraceRec* T, bool by_level, float* res3,
                             int* iterations, double* trace_d, float* trace_f, int* trace_records) {
  int written = 0;
  for (int p = 0; p < P; p++) {
    lv[p].m->resident->st.settled();
    const int at = by_level ? lv[p].lvl : 0;
    if (res3) for (int k = 0; k < 3; k++) res3[3 * at + k] = O[p].res3[k];
    if (iterations) iterations[at] = O[p].iterations;
    if (trace_d)
      for (int k = 0; k < O[p].tests; k++, written++) {
        const dmv::InitLmTraceRec& R = T[Q[p].trace_base + k];
        memcpy(trace_d + (size_t)written * dmv::INIT_LM_TRACE_D, R.d, sizeof(R.d));
        memcpy(trace_f + (size_t)written * dmv::INIT_LM_TRACE_F, R.f, sizeof(R.f));
      }
  }
  if (trace_d) *trace_records = written;
}
