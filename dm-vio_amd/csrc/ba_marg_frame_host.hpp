// ================================================================================================= frame marginalisation, W windows per call
// dmvio_hip_ba_marginalize_frame (capi_ba.hip: BAHost::marginalizeFrame on the host, per window) for W windows: EnergyFunctional::marginalizeFrame's visual-only branch
// (EnergyFunctional.cpp:570-640).  The windows are ordered by keyframe count (the caller's order inside a count); every window's prior, the frame's prior / delta_prior and
// (F, frame) are packed into the pinned half of the batch's marginalisation buffer at one stride and go up in ONE copy; one launch of k_ba_marg_frame_b per count
// (ba_marg_frame_kernels.hpp: one workgroup per window); the reduced priors come back in ONE copy behind ONE wait and are scattered into the callers' arrays.  Like the
// single call it changes nothing in the handles.
// Part of capi_ba.hip's unit: included by ba_batch_host.hpp behind the batch object and its buffers.
#pragma once
#include "ba_marg_frame_kernels.hpp"

struct MargFrameBatchCall {
  dmvio_hip_ba_batch* const B;
  const int W;
  dmvio_hip_ba_marg_frame_window* const win;
  std::vector<int> order;                    // record k holds window order[k]
  struct Grp { int w0, cnt, F; };
  std::vector<Grp> grp;
  size_t inStride = 0, outStride = 0;        // doubles per record: the call's largest window
  size_t inBytes = 0, outBytes = 0;
  MargFrameBatchCall(dmvio_hip_ba_batch* B_, const int W_, dmvio_hip_ba_marg_frame_window* win_) : B(B_), W(W_), win(win_) {}

  // k_ba_marg_frame_b keeps a window's n x n system in LDS: 88 KB at 12 keyframes, above the 64 KB a launch gets without asking.  Once per batch object: the device's
  // limit, and the kernel's attribute raised to what the largest window needs (or to the limit, where that is less: the windows that fit still run)
  int allowLds(const size_t need) {
    if (!B->margf_lds_limit) {
      int lim = 0;
      HIPCHK(hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, B->ctx->device));
      if (lim <= 0) return failmsg("ba_marginalize_frame_batch: the device reports no LDS per workgroup");
      const size_t most = sizeof(double) * dmv::baMargFrameLdsDoubles(BA_BATCH_NMAX);
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&dmv::k_ba_marg_frame_b), hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::min<size_t>(most, (size_t)lim)));
      B->margf_lds_limit = (size_t)lim;
    }
    if (need > B->margf_lds_limit)
      return failmsg("ba_marginalize_frame_batch: a window of the call needs " + std::to_string(need) + " bytes of LDS per workgroup, the device allows " +
                     std::to_string(B->margf_lds_limit));
    return 0;
  }

  int plan() {
    std::vector<char> done(W, 0);
    int Fmax = 0;
    for (int i = 0; i < W; i++) {
      if (done[i]) continue;
      Grp g{(int)order.size(), 0, win[i].ba->H.F};
      for (int j = i; j < W; j++) if (!done[j] && win[j].ba->H.F == g.F) { order.push_back(j); done[j] = 1; g.cnt++; }
      grp.push_back(g);
      Fmax = std::max(Fmax, g.F);
    }
    const int nmax = 4 + 8 * Fmax;
    if (int r = allowLds(sizeof(double) * dmv::baMargFrameLdsDoubles(nmax))) return r;
    inStride = dmv::baMargFrameInDoubles(nmax); outStride = dmv::baMargFrameOutDoubles(nmax);
    DmvCursor C;   // [W records in | W records out]: the marginalisation buffer of MargBatchCall, grown as there and kept for the calls that follow
    C.take<double>(inStride * W);
    inBytes = C.bytes();
    C.take<double>(outStride * W);
    outBytes = C.bytes() - inBytes;
    return B->margBegin(C.bytes(), &B->margf_work);
  }

  // ---- record k in the pinned buffer: [HM | bM | prior | delta_prior] at the window's own n, (F, frame) in the stride's last double.  A handle without a prior: zeros
  int fillWindow(const int k) {
    const dmvio_hip_ba_marg_frame_window& q = win[order[k]];
    const BAHost& H = q.ba->H;
    const size_t n = (size_t)H.n();
    double* rec = B->marg.host<double>(0) + inStride * k;
    if (H.HM.size() == n * n) { memcpy(rec, H.HM.data(), sizeof(double) * n * n); memcpy(rec + n * n, H.bM.data(), sizeof(double) * n); }
    else memset(rec, 0, sizeof(double) * (n * n + n));
    const BAFrameHost& fr = H.fr[q.frame];
    memcpy(rec + n * n + n, fr.prior, sizeof(double) * 8); memcpy(rec + n * n + n + 8, fr.delta_prior, sizeof(double) * 8);
    int* hdr = reinterpret_cast<int*>(rec + inStride - 1);
    hdr[0] = H.F; hdr[1] = q.frame;
    return 0;
  }

  int enqueue() {
    const hipStream_t s = B->stream;
    DmvWork& work = B->margf_work;
    // a handle's own stream may still hold work: in front of the call (as MargBatchCall::enqueue)
    for (int k = 0; k < W; k++) {
      dmvio_hip_ba* b = win[order[k]].ba;
      if (b->stream == s || hipStreamQuery(b->stream) == hipSuccess) continue;
      HIPCHK(hipEventRecord(B->marg_ev, b->stream));
      HIPCHK(hipStreamWaitEvent(s, B->marg_ev, 0));
    }
    (void)hipGetLastError();   // (hipErrorNotReady of the query above is no error)
    if (B->profile) HIPCHK(hipEventRecord(B->ev[6], s));
    const double* d_in = B->marg.dev<const double>(0);
    double* d_out = B->marg.dev<double>(inBytes);
    if (int r = B->marg.upload(s, inBytes)) return r;
    for (const Grp& g : grp) {
      const size_t lds = sizeof(double) * dmv::baMargFrameLdsDoubles(4 + 8 * g.F);
      hipLaunchKernelGGL(dmv::k_ba_marg_frame_b, dim3(g.cnt), dim3(dmv::BA_MARGF_THREADS), lds, s, d_in, d_out, inStride, outStride, g.w0);
      work.launches++;
      HIPCHK(hipGetLastError());
    }
    if (int r = B->marg.download(s, inBytes, outBytes)) return r;
    if (B->profile) HIPCHK(hipEventRecord(B->ev[7], s));
    if (int r = B->marg.wait(s)) return r;
    B->margf_ms = 0;
    if (B->profile) HIPCHK(hipEventElapsedTime(&B->margf_ms, B->ev[6], B->ev[7]));
    return 0;
  }

  int scatterWindow(const int k) {
    const dmvio_hip_ba_marg_frame_window& q = win[order[k]];
    const size_t nd = (size_t)q.ba->H.n() - 8;
    const double* res = B->marg.host<const double>(inBytes) + outStride * k;
    memcpy(q.HM_new, res, sizeof(double) * nd * nd); memcpy(q.bM_new, res + nd * nd, sizeof(double) * nd);
    return 0;
  }
};

extern "C" {
int dmvio_hip_ba_marginalize_frame_batch(dmvio_hip_ba_batch* B, int W, dmvio_hip_ba_marg_frame_window* win) {
  if (!B) return failmsg("ba_marginalize_frame_batch: null batch");
  if (W < 0) return failmsg("ba_marginalize_frame_batch: W < 0");
  if (W > B->cap) return failmsg("ba_marginalize_frame_batch: more windows than the batch was created for");
  std::lock_guard<std::mutex> lkB(B->mu);
  if (W == 0) { B->margf_work.clear(); B->margf_ms = 0; return 0; }
  if (!win) return failmsg("ba_marginalize_frame_batch: null window list");
  std::vector<dmvio_hip_ba*> order(W);
  for (int i = 0; i < W; i++) {
    if (!win[i].ba) return failmsg("ba_marginalize_frame_batch: null window");
    if (!win[i].HM_new || !win[i].bM_new) return failmsg("ba_marginalize_frame_batch: null HM_new / bM_new");
    if (win[i].ba->ctx != B->ctx) return failmsg("ba_marginalize_frame_batch: a window belongs to another context");
    order[i] = win[i].ba;
  }
  // the handles' locks, in address order (as dmvio_hip_ba_marginalize_points_batch)
  if (dmvFirstRepeated(win, W, &dmvio_hip_ba_marg_frame_window::ba) >= 0) return failmsg("ba_marginalize_frame_batch: a window appears twice");
  std::sort(order.begin(), order.end());
  std::vector<std::unique_lock<std::recursive_mutex>> locks;
  for (dmvio_hip_ba* b : order) locks.emplace_back(b->mu);
  for (int i = 0; i < W; i++) {
    const dmvio_hip_ba* b = win[i].ba;
    if (b->H.F < 1) return failmsg("ba_marginalize_frame_batch: a handle without a window (dmvio_hip_ba_set_window first)");
    if (win[i].frame < 0 || win[i].frame >= b->H.F) return failmsg("ba_marginalize_frame_batch: frame " + std::to_string(win[i].frame) + " of window " + std::to_string(i) + " out of range");
    if (sharded(b)) return failmsg("ba_marginalize_frame_batch: a window sharded over ranks cannot join a batch");
  }
  HIPCHK(hipSetDevice(B->ctx->device));
  MargFrameBatchCall c(B, W, win);
  if (int r = c.plan()) return r;
  B->margf_work.clear();
  if (int r = B->workers.parallelFor(W, [&c](const int k) { return c.fillWindow(k); })) return r;
  if (int r = c.enqueue()) return r;
  return B->workers.parallelFor(W, [&c](const int k) { return c.scatterWindow(k); });
}
int dmvio_hip_ba_batch_last_marg_frame_ms(dmvio_hip_ba_batch* B, float* ms) {
  if (!B || !ms) return failmsg("ba_batch_last_marg_frame_ms: null argument");
  std::lock_guard<std::mutex> lkB(B->mu);
  *ms = B->margf_ms;
  return 0;
}
int dmvio_hip_ba_batch_last_marg_frame_work(dmvio_hip_ba_batch* B, int* launches, int* uploads, int* downloads, int* waits) {
  if (!B) return failmsg("ba_batch_last_marg_frame_work: null batch");
  std::lock_guard<std::mutex> lkB(B->mu);
  B->margf_work.report(launches, uploads, downloads, waits);
  return 0;
}
}  // extern "C"
