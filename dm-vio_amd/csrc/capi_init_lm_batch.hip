// C ABI of the initializer's LM loop, the frames of W windows per call (include/dmvio_hip_init_lm_batch.h): CoarseInitializer::trackFrame
// (src/dso/FullSystem/CoarseInitializer.cpp:85-281) on the resident point sets of capi_init_resident.hip, one workgroup per window.  This unit checks the call — per window by
// the single call's own lmCheck, across the windows (a handle or a state slot named twice) itself — keeps the batch's LM records and enqueues ONE launch of
// k_init_lm_frame_b (init_lm_batch_kernels.hpp).  A window's levels, its records, their upload and the delivery of its results are the single call's (init_lm_host.hpp).
#include <vector>
#include <cstring>
#include <cstdio>
#include <algorithm>
#include "../../include/dmvio_hip_init_lm_batch.h"
#include "init_lm_host.hpp"
#include "init_lm_batch_kernels.hpp"

using namespace dmv;

// `slab`, per call: [InitLmWin x W | InitLmProb x levels of the call | incoming states x W || outgoing states x W | InitLmOut x levels | trace records].  An upload covers the
// records, or the records and the incoming states; the download is everything behind `||`.  `sent`: the records as the device holds them — a call whose records equal them
// and that brings no state uploads nothing.  `records`: the LM records, one per state slot, device only; `filled`: the slots that hold a state.
struct dmvio_hip_initializer_lm_batch {
  dmvio_hip_ctx* ctx = nullptr;   // the owner: every call locks its `mu`
  int max_windows = 0;
  DmvSlab slab, records;
  DmvWork work;
  std::vector<char> sent;
  std::vector<char> filled;
  size_t lds_limit = 0, lds_static = 0;
};

extern "C" {

dmvio_hip_initializer_lm_batch* dmvio_hip_initializer_lm_batch_create(dmvio_hip_ctx* ctx, int max_windows) {
  if (!ctx || max_windows < 1 || max_windows > 65535) { failmsg("initializer_lm_batch_create: bad argument (max_windows in [1, 65535]: the window is a grid dimension)"); return nullptr; }
  auto bad = [](hipError_t e) { if (e != hipSuccess) failmsg(std::string("initializer_lm_batch_create: ") + hipGetErrorString(e)); return e != hipSuccess; };
  if (bad(hipSetDevice(ctx->device))) return nullptr;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int lim = 0;
  size_t own = 0;
  if (bad(initLdsAllow(ctx->device, &lim, reinterpret_cast<const void*>(&k_init_lm_frame_b), &own))) return nullptr;
  if (lim <= 0 || own >= (size_t)lim) { failmsg("initializer_lm_batch_create: the kernel's own LDS exceeds what the device allows a workgroup"); return nullptr; }
  dmvio_hip_initializer_lm_batch* b = new dmvio_hip_initializer_lm_batch();
  b->ctx = ctx; b->max_windows = max_windows;
  b->lds_limit = (size_t)lim; b->lds_static = own;
  b->filled.assign((size_t)max_windows, 0);
  b->slab.work = &b->work;
  // the slab for up to 64 three-level windows without a trace; a call that needs more grows it (DmvSlab::reserve)
  const int W0 = std::min(max_windows, 64);
  DmvCursor cur;
  dmvRecords(cur, sizeof(InitLmWin), W0); cur.take<InitLmProb>(3 * (size_t)W0); cur.take<InitLmState>(W0);
  cur.take<InitLmState>(W0); cur.take<InitLmOut>(3 * (size_t)W0);
  if (b->records.create(sizeof(InitLmState) * (size_t)max_windows, 0) || b->slab.create(cur.bytes())) {
    b->records.release(); b->slab.release();
    delete b;
    return nullptr;
  }
  return b;
}

void dmvio_hip_initializer_lm_batch_destroy(dmvio_hip_initializer_lm_batch* b) {
  if (!b) return;
  hipSetDevice(b->ctx->device);
  {
    std::lock_guard<std::mutex> lk(b->ctx->mu);
    hipStreamSynchronize(b->ctx->stream);
    b->slab.release(); b->records.release();
  }
  delete b;
}

int dmvio_hip_initializer_resident_track_frame_batch(dmvio_hip_initializer_lm_batch* b, int W, dmvio_hip_initializer_lm_window* win) {
  static const char* who = "initializer_resident_track_frame_batch";
  if (int r = dmvBatchHead(b, W, b ? b->max_windows : 0, win, who)) return r;
  if (W == 0) return 0;
  dmvio_hip_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  char msg[200], at[96];

  // ---- the whole call is checked before anything is written or enqueued
  std::vector<const void*> handles;
  std::vector<int> handle_win, first_prob((size_t)W + 1, 0);
  for (int i = 0; i < W; i++) {
    const dmvio_hip_initializer_lm_window& w = win[i];
    auto no = [&](const char* what) { snprintf(msg, sizeof(msg), "%s: window %d: %s", who, i, what); return failmsg(msg); };
    if (!w.levels) return no("null handle array");
    if (w.n_levels < 1 || w.n_levels > c->levels) { snprintf(msg, sizeof(msg), "%s: window %d: n_levels = %d outside [1, %d], the context's levels", who, i, w.n_levels, c->levels); return failmsg(msg); }
    for (int k = 0; k < w.n_levels; k++) {
      if (!w.levels[k]) { snprintf(msg, sizeof(msg), "%s: window %d: null initializer handle of level %d", who, i, k); return failmsg(msg); }
      if (w.levels[k]->ctx != c) { snprintf(msg, sizeof(msg), "%s: window %d: the handle of level %d belongs to another context than the batch's", who, i, k); return failmsg(msg); }
      handles.push_back(w.levels[k]); handle_win.push_back(i);
    }
    if (!w.Ki9_levels || !w.fxfycxcy_levels || !w.max_iterations) return no("null argument");
    if (!w.state_out10) return no("state_out10 is NULL");
    if (w.state_slot < 0 || w.state_slot >= b->max_windows) { snprintf(msg, sizeof(msg), "%s: window %d: state_slot = %d outside [0, %d)", who, i, w.state_slot, b->max_windows); return failmsg(msg); }
    first_prob[(size_t)i + 1] = first_prob[i] + w.n_levels;
  }
  {
    const int rep = dmvFirstRepeated(handles.data(), (int)handles.size());
    if (rep >= 0) {
      int j = 0;
      while (handles[j] != handles[rep]) j++;
      snprintf(msg, sizeof(msg), "%s: window %d: the handle of level %d is the handle of level %d of window %d named again", who, handle_win[rep], rep - first_prob[handle_win[rep]],
               j - first_prob[handle_win[j]], handle_win[j]);
      return failmsg(msg);
    }
    std::vector<int> slot_win((size_t)b->max_windows, -1);
    for (int i = 0; i < W; i++) {
      int& first = slot_win[win[i].state_slot];
      if (first >= 0) { snprintf(msg, sizeof(msg), "%s: window %d: state_slot %d is window %d's", who, i, win[i].state_slot, first); return failmsg(msg); }
      first = i;
    }
  }
  const int total = first_prob[W];
  std::vector<LmLevel> lv((size_t)total);
  std::vector<LmCommon> K((size_t)W);
  std::vector<int> trace_base((size_t)W + 1, 0);
  int most = 0;
  bool any_in = false;
  for (int i = 0; i < W; i++) {
    const dmvio_hip_initializer_lm_window& w = win[i];
    LmLevel* v = lv.data() + first_prob[i];
    const int tests = lmFrameLevels(v, w.levels, w.n_levels, w.max_iterations, w.Ki9_levels, w.fxfycxcy_levels);
    K[i] = {w.first_slot, w.new_slot, w.fix_affine != 0, w.alphaW, w.alphaK, w.regWeight, w.couplingWeight, w.priorY, w.priorX, w.wM8};
    snprintf(at, sizeof(at), "%s: window %d", who, i);
    const LmLimits lim = {b->lds_static, b->lds_limit, b->filled[w.state_slot] != 0, "the batch's record of this state_slot"};
    if (int r = lmCheck(at, c, lim, v, w.n_levels, K[i], w.state_in10, w.trace_capacity, w.trace_d, w.trace_f, w.trace_records, nullptr)) return r;
    for (int p = 0; p < w.n_levels; p++) most = std::max(most, v[p].m->resident->n);
    trace_base[(size_t)i + 1] = trace_base[i] + (w.trace_d ? tests : 0);   // (lmCheck has held max_iterations to [0, 64])
    any_in = any_in || w.state_in10;
  }

  // ---- the records
  hipStream_t s = c->stream;
  for (int i = 0; i < W; i++) { if (int r = dmv_ensure_row_major_locked(c, win[i].first_slot)) return r; if (int r = dmv_ensure_row_major_locked(c, win[i].new_slot)) return r; }   // (not counted, as in the single call)
  DmvCursor cur;
  const size_t o_win = dmvRecords(cur, sizeof(InitLmWin), W), o_prob = cur.take<InitLmProb>(total);
  const size_t rec_bytes = cur.bytes();
  const size_t o_sin = cur.take<InitLmState>(W);
  const size_t up_bytes = cur.bytes();
  const size_t o_sout = cur.take<InitLmState>(W), o_outs = cur.take<InitLmOut>(total), o_trace = cur.take<InitLmTraceRec>(trace_base[W]);
  const size_t down_end = o_trace + sizeof(InitLmTraceRec) * (size_t)trace_base[W];
  std::vector<char> rec(rec_bytes, 0);
  InitLmWin* HW = reinterpret_cast<InitLmWin*>(rec.data() + o_win);
  InitLmProb* Q = reinterpret_cast<InitLmProb*>(rec.data() + o_prob);
  for (int i = 0; i < W; i++) {
    const dmvio_hip_initializer_lm_window& w = win[i];
    InitLmWin& H = HW[i];
    H.n_levels = w.n_levels; H.prob_base = first_prob[i]; H.state_slot = w.state_slot; H.traced = w.trace_d != nullptr;
    int tb = trace_base[i];
    for (int p = 0; p < w.n_levels; p++) {
      const LmLevel& v = lv[(size_t)first_prob[i] + p];
      lmFillProb(Q[first_prob[i] + p], c, v, K[i], first_prob[i] + p, tb);
      tb += v.max_iterations + 1;
      if (p > 0) {
        const DmvInitResident* R = v.m->resident;
        H.parent[p] = R->i(R->o_parent); H.child_begin[p] = R->i(R->o_cbegin); H.children[p] = R->i(R->o_children); H.n_listed[p] = R->n_listed;
      }
    }
  }
  if (cur.bytes() > b->slab.cap) {   // growing drops what the device held of the records
    if (int r = b->slab.reserve(cur.bytes(), cur.bytes() + cur.bytes() / 2, s)) return r;
    b->sent.clear();
  }
  b->work.clear();
  if (int r = lmSend(b->slab, b->sent, rec, any_in, any_in ? up_bytes : rec_bytes, s, [&] {
        InitLmState* S = b->slab.host<InitLmState>(o_sin);
        for (int i = 0; i < W; i++) {
          if (win[i].state_in10) { lmStateFrom10(S + i, win[i].state_in10); S[i].pad = 1; }
          else memset(S + i, 0, sizeof(InitLmState));
        }
      })) return r;
  for (int i = 0; i < W; i++) if (win[i].state_in10) b->filled[win[i].state_slot] = 1;

  // ---- ONE launch, ONE download, ONE wait
  hipLaunchKernelGGL(k_init_lm_frame_b, dim3((unsigned)W), dim3(256), resSweepLds(most), s, b->slab.dev<const InitLmWin>(o_win), b->slab.dev<const InitLmProb>(o_prob),
                     b->records.dev<InitLmState>(0), any_in ? b->slab.dev<const InitLmState>(o_sin) : nullptr, b->slab.dev<InitLmState>(o_sout), b->slab.dev<InitLmOut>(o_outs),
                     b->slab.dev<InitLmTraceRec>(o_trace));
  b->work.launches++;
  HIPCHK(hipGetLastError());
  if (int r = b->slab.download(s, o_sout, down_end - o_sout)) return r;
  if (int r = b->slab.wait(s)) return r;
  const InitLmState* S = b->slab.host<InitLmState>(o_sout);
  const InitLmOut* O = b->slab.host<InitLmOut>(o_outs);
  const InitLmTraceRec* T = b->slab.host<InitLmTraceRec>(o_trace);
  for (int i = 0; i < W; i++) {
    dmvio_hip_initializer_lm_window& w = win[i];
    lmStateTo10(S + i, w.state_out10);
    w.snapped = S[i].snapped ? 1 : 0;
    const int q = first_prob[i];
    lmDeliver(lv.data() + q, w.n_levels, Q + q, O + q, T, true, w.res3_levels, w.iterations_levels, w.trace_d, w.trace_f, w.trace_records);
  }
  return 0;
}

int dmvio_hip_initializer_lm_batch_last_work(dmvio_hip_initializer_lm_batch* b, int* launches, int* uploads, int* downloads, int* waits) {
  if (!b) return failmsg("initializer_lm_batch_last_work: null batch handle");
  std::lock_guard<std::mutex> lk(b->ctx->mu);
  b->work.report(launches, uploads, downloads, waits);
  return 0;
}

}  // extern "C"
