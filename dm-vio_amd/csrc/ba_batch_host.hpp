// ================================================================================================= device-resident Gauss-Newton loop, W windows per launch (round 5)
// FullSystem::optimize (FullSystemOptimize.cpp:417-647) for W windows at once, the reference's non-GTSAM solver branch: per Gauss-Newton iteration the host enqueues ONE
// fixed sequence of kernels for all windows (ba_batch_kernels.hpp) and never waits — the 68x68 solve, the frame step, the pair tables, the energies and the accept test run
// on the device (k_ba_solve + the decision pass of the linearisation), every kernel of the chain takes its window from blockIdx.y and is gated on that window's own decision.
// Two waits per call: behind the loop (the frame states come back, the host re-anchors the newest keyframe, FullSystemOptimize.cpp:596-603) and behind the final
// fix-linearisation.  Windows of one call must hold the same number of keyframes (the adjoint stitch's workgroup shape); the caller groups them.
// the per-window host work of a batch call (tables, nullspace bases, staging copies before the launches; state write-back, adjoints and pair tables behind the loop:
// 30-40 us per window each) is dealt out over a few persistent worker threads — at 64 windows it was 4.3 ms of a 12 ms call
//
// The host side only, and part of capi_ba.hip's translation unit: included there, once, behind the handle's helpers it uses (fillWindow, dynFromHost, makeDecide, resolveTh,
// uploadAdjoints, BA_BY_MAXF; calcLEnergy of ba_loop_host.hpp; accumArgs / accBlocks of the handle).  The BA device code stays in that one unit in its include order — a second unit that instantiated the batched kernels compiled
// three of them differently.
#pragma once
#include <thread>
#include <condition_variable>
struct BAWorkers {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv, cv_done;
  std::function<int(int)> fn;
  int next = 0, count = 0, pending = 0, rc = 0, device = 0;
  unsigned long long gen = 0;
  bool quit = false;
  std::string err;
  void start(int n, int dev) {
    device = dev;
    for (int i = 0; i < n; i++) th.emplace_back([this] { run(); });
  }
  void run() {
    hipSetDevice(device);
    unsigned long long seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return quit || (gen != seen && next < count); });
      if (quit) return;
      while (next < count) {
        const int i = next++;
        lk.unlock();
        const int r = fn(i);
        std::string e = r ? dmv_err() : std::string();
        lk.lock();
        if (r && !rc) { rc = r; err = e; }
        if (--pending == 0) cv_done.notify_all();
      }
      seen = gen;
    }
  }
  // fn(i) for i in [0, n): on the workers and on the calling thread; returns the first non-zero result (its message becomes this thread's last error)
  int parallelFor(int n, std::function<int(int)> f, const int serial_below = 8) {
    if (th.empty() || n < serial_below) { for (int i = 0; i < n; i++) if (int r = f(i)) return r; return 0; }
    {
      std::lock_guard<std::mutex> lk(mu);
      fn = std::move(f); next = 0; count = n; pending = n; rc = 0; gen++;
    }
    cv.notify_all();
    for (;;) {
      std::unique_lock<std::mutex> lk(mu);
      if (next >= count) { cv_done.wait(lk, [&] { return pending == 0; }); break; }
      const int i = next++;
      lk.unlock();
      const int r = fn(i);
      std::string e = r ? dmv_err() : std::string();
      lk.lock();
      if (r && !rc) { rc = r; err = e; }
      if (--pending == 0) cv_done.notify_all();
    }
    if (rc) { dmv_err() = err; dmv_err_epoch()++; }
    return rc;
  }
  // fn(i) for i in [0, n), handed out in index order, on the workers ALONE: the caller goes on (it enqueues one group's launches while the next group's tables are prepared)
  // and collects the result with waitAsync().  Needs workers (th.empty(): use parallelFor).
  void startAsync(int n, std::function<int(int)> f) {
    {
      std::lock_guard<std::mutex> lk(mu);
      fn = std::move(f); next = 0; count = n; pending = n; rc = 0; gen++;
    }
    cv.notify_all();
  }
  int waitAsync(const bool report = true) {   // report = false: on the caller's own error path — wait only, its error message stays
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return pending == 0; });
    if (rc && report) { dmv_err() = err; dmv_err_epoch()++; }
    return rc;
  }
  ~BAWorkers() {
    { std::lock_guard<std::mutex> lk(mu); quit = true; }
    cv.notify_all();
    for (auto& t : th) t.join();
  }
};
static constexpr int BA_BATCH_NMAX = 4 + 8 * BA_MAXF_CAP;
// The layout of a window's piece of the batch's three slabs, for windows of F keyframes / n = 4 + 8 F unknowns.  (BA_BATCH_NMAX, BA_MAXF_CAP) gives the strides the slabs
// are allocated with, a call's (n, F) where its windows' parts lie inside them.
//   tables (uploaded; byte offsets)    [HM n x n | bM n | basis 7 x n] doubles, [adHostF F2 x 64 | adTargetF F2 x 64] floats, [pre F2] BAPrecalc
//   device output (offsets in doubles) [sys 2 (n x n + n) | resInA | trace 64 x 4 | x_last BA_BATCH_NMAX | sysL n x n + n]: H_L, b_L of the residuals kept linearised last
//   pinned mirror (offsets in doubles) [resInA | trace | x_last]: the middle of the device output, what comes back behind the loop
struct BatchLayout {
  enum : size_t { TRACE = 64 * 4, MIRROR_TRACE = 1, MIRROR_XLAST = 1 + TRACE, MIRROR_STRIDE = 1 + TRACE + BA_BATCH_NMAX };
  const size_t n, F2;
  BatchLayout(const int n_, const int F_) : n((size_t)n_), F2((size_t)F_ * F_) {}
  static size_t padded(const size_t bytes) { return dmvPad(bytes); }
  size_t tabHM() const { return 0; }
  size_t tabBM() const { return sizeof(double) * n * n; }
  size_t tabBasis() const { return tabBM() + sizeof(double) * n; }
  size_t tabAdBytes() const { return sizeof(float) * F2 * 64; }
  size_t tabAdHostF() const { return tabBasis() + sizeof(double) * 7 * n; }
  size_t tabAdTargetF() const { return tabAdHostF() + tabAdBytes(); }
  size_t tabPre() const { return tabAdTargetF() + tabAdBytes(); }
  size_t tabPreBytes() const { return sizeof(BAPrecalc) * F2; }
  size_t tabUsed() const { return tabPre() + tabPreBytes(); }
  size_t tabStride() const { return padded(tabUsed()); }
  size_t sysLDoubles() const { return n * n + n; }
  size_t outResInA() const { return 2 * (n * n + n); }
  size_t outTrace() const { return outResInA() + 1; }
  size_t outXLast() const { return outTrace() + TRACE; }
  size_t outSysL() const { return outXLast() + BA_BATCH_NMAX; }
  size_t outStride() const { return padded(sizeof(double) * (outSysL() + sysLDoubles())); }
  size_t mirrorUsed() const { return MIRROR_XLAST + n; }
  bool fitsIn(const BatchLayout& cap) const { return tabUsed() <= cap.tabStride() && outStride() <= cap.outStride() && mirrorUsed() <= MIRROR_STRIDE; }
  // ---- dmvio_hip_ba_marginalize_points_batch in the same slabs (a call owns them from its first line to its last wait: the batch's lock)
  //   tables (byte offsets)              [pre F2 | adHost F2 x 64 | adTarget F2 x 64 doubles]: the adjoints only of a window whose device copy is stale
  //   marginalisation buffer (bytes)     [candidates of every window, N bytes each, padded] then per window [sys 2 (n x n + n) | resInA doubles | decisions N bytes, padded]:
  //                                      the first part goes up in one copy, the second comes back in one
  size_t margTabPre() const { return 0; }
  size_t margTabAdBytes() const { return sizeof(double) * F2 * 64; }
  size_t margTabAdHost() const { return padded(tabPreBytes()); }
  size_t margTabAdTarget() const { return margTabAdHost() + margTabAdBytes(); }
  size_t margTabUsed(const bool adjoints) const { return adjoints ? margTabAdTarget() + margTabAdBytes() : tabPreBytes(); }
  size_t margSysDoubles() const { return outResInA() + 1; }
  size_t margOutDecision() const { return sizeof(double) * margSysDoubles(); }
  bool margFitsIn(const BatchLayout& cap) const { return margTabUsed(true) <= cap.tabStride(); }
};
struct dmvio_hip_ba_batch {
  BAWorkers workers;
  dmvio_hip_ctx* ctx = nullptr;
  hipStream_t stream = nullptr;
  int cap = 0;
  std::mutex mu;
  BAWinDev* d_wins = nullptr;
  BAWinDev* h_wins = nullptr;      // pinned
  // the three slabs (BatchLayout), `cap` windows each at the strides of `slab`
  const BatchLayout slab{BA_BATCH_NMAX, BA_MAXF_CAP};
  char* d_tab = nullptr;           // the tables, uploaded
  char* h_tab = nullptr;           // ... and where they are filled: pinned
  char* d_out = nullptr;           // the device output (device-only but for its mirrored part)
  double* h_trace = nullptr;       // the mirror: pinned
  char* dTab(const int w) const { return d_tab + slab.tabStride() * (size_t)w; }
  char* hTab(const int w) const { return h_tab + slab.tabStride() * (size_t)w; }
  double* dOut(const int w) const { return reinterpret_cast<double*>(d_out + slab.outStride() * (size_t)w); }
  double* hMirror(const int w) const { return h_trace + (size_t)BatchLayout::MIRROR_STRIDE * w; }
  int exact_backsub = 0;
  double host_us[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // host clock of the last call's phases (dmvio_hip_ba_batch_last_host_us)
  float last_ms[3] = {0, 0, 0};    // HIP-event times of the last call: the loop (init chain + iterations), the final fix-linearisation, [profile] one stepped linearisation
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // a batch of >= 4 windows is cut into groups (three by default, at most BA_BATCH_STREAMS), one stream each, their launches interleaved stage by stage (optimizeBatchGroup): while one group's
  // k_ba_solve runs (one workgroup per window) the other groups' linearisations / accumulations fill the device
  enum { BA_BATCH_STREAMS = 8 };
  hipStream_t gstream[BA_BATCH_STREAMS] = {};   // [0] = stream
  hipEvent_t gev[BA_BATCH_STREAMS][3] = {};                                        // per group: [0] its initial linearisation is enqueued (the next group's start), [1] its loop is done and its states are on the host, [2] its last kernel
  int lin_lanes = 1;               // dmvio_hip_ba_batch_set_linearize_lanes: 1 = k_ba_linearize_b1 (one lane per residual) from 4 windows on, 8 = always the eight-lane kernel
  int streams = 0;                 // dmvio_hip_ba_batch_set_streams: 0 = automatic, k >= 1 = at most k groups (1: the whole batch on one stream)
  int profile = 0;                 // dmvio_hip_ba_batch_set_profile: events around the stepped linearisation of iteration 1 (k_ba_linearize_b of all windows)
  // dmvio_hip_ba_marginalize_points_batch: the candidates / systems / decisions of a call (BatchLayout), device and pinned, grown on demand to twice the need and kept
  // (batch_slab.hpp); the event that puts a handle's own pending work in front of the call; what the last call enqueued
  DmvSlab marg;
  hipEvent_t marg_ev = nullptr;
  DmvWork marg_work;
  // the marginalisation buffer holds `bytes` and its pinned side is free to write; `work` counts what the call does with it
  int margBegin(const size_t bytes, DmvWork* work) {
    if (int r = marg.reserve(bytes, bytes * 2, stream)) return r;
    if (!marg_ev) HIPCHK(hipEventCreateWithFlags(&marg_ev, hipEventDisableTiming));
    marg.work = work;
    return marg.begin(stream);
  }
  float marg_ms = 0;                 // with `profile`: HIP events around the last call's device work (first upload .. the download)
  // dmvio_hip_ba_marginalize_frame_batch: in the same buffers (a call owns them under the batch's lock); the most dynamic LDS a launch may ask for on this device
  // (0: not asked yet — k_ba_marg_frame_b's attribute is set with the first call)
  DmvWork margf_work;
  float margf_ms = 0;
  size_t margf_lds_limit = 0;
  // dmvio_hip_ba_set_graph_from_batch (ba_graph_batch_host.hpp): the call's records, range / piece tables and flattened graphs, pinned and on the device, grown on demand
  // and kept like the marginalisation buffer; what the last call enqueued
  DmvSlab graph;
  DmvWork graph_work;
  float graph_ms = 0;                 // with `profile`: HIP events from the upload to the last kernel
};
extern "C" {
dmvio_hip_ba_batch* dmvio_hip_ba_batch_create(dmvio_hip_ctx* ctx, int max_windows) {
  if (!ctx || max_windows < 1 || max_windows > 4096) { failmsg("ba_batch_create: bad argument"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { failmsg("ba_batch_create: hipSetDevice failed"); return nullptr; }
  dmvio_hip_ba_batch* B = new dmvio_hip_ba_batch();
  B->ctx = ctx; B->cap = max_windows;
  bool ok = hipStreamCreateWithFlags(&B->stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipMalloc((void**)&B->d_wins, sizeof(BAWinDev) * max_windows) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&B->h_wins, sizeof(BAWinDev) * max_windows, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipMalloc((void**)&B->d_tab, B->slab.tabStride() * max_windows) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&B->h_tab, B->slab.tabStride() * max_windows, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipMalloc((void**)&B->d_out, B->slab.outStride() * max_windows) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&B->h_trace, sizeof(double) * BatchLayout::MIRROR_STRIDE * max_windows, hipHostMallocDefault) == hipSuccess;
  for (int k = 0; k < 8 && ok; k++) ok = hipEventCreate(&B->ev[k]) == hipSuccess;
  B->gstream[0] = B->stream;
  for (int g = 1; g < dmvio_hip_ba_batch::BA_BATCH_STREAMS && ok; g++) ok = hipStreamCreateWithFlags(&B->gstream[g], hipStreamNonBlocking) == hipSuccess;
  for (int g = 0; g < dmvio_hip_ba_batch::BA_BATCH_STREAMS && ok; g++) for (int k = 0; k < 3 && ok; k++) ok = hipEventCreateWithFlags(&B->gev[g][k], hipEventDisableTiming) == hipSuccess;
  if (ok) ok = hipMemset(B->d_out, 0, B->slab.outStride() * max_windows) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
  if (!ok) { failmsg("ba_batch_create: device / pinned allocation failed"); dmvio_hip_ba_batch_destroy(B); return nullptr; }
  if (max_windows >= 8) {
    const unsigned int hw = std::thread::hardware_concurrency();
    B->workers.start((int)std::min<unsigned int>(7, hw > 2 ? hw - 2 : 0), ctx->device);
  }
  return B;
}
void dmvio_hip_ba_batch_destroy(dmvio_hip_ba_batch* B) {
  if (!B) return;
  hipSetDevice(B->ctx->device);
  if (B->stream) { hipStreamSynchronize(B->stream); hipStreamDestroy(B->stream); }
  if (B->d_wins) hipFree(B->d_wins);
  if (B->h_wins) hipHostFree(B->h_wins);
  if (B->d_tab) hipFree(B->d_tab);
  if (B->h_tab) hipHostFree(B->h_tab);
  if (B->d_out) hipFree(B->d_out);
  if (B->h_trace) hipHostFree(B->h_trace);
  B->marg.release(); B->graph.release();
  if (B->marg_ev) hipEventDestroy(B->marg_ev);
  for (int k = 0; k < 8; k++) if (B->ev[k]) hipEventDestroy(B->ev[k]);
  for (int g = 1; g < dmvio_hip_ba_batch::BA_BATCH_STREAMS; g++) if (B->gstream[g]) { hipStreamSynchronize(B->gstream[g]); hipStreamDestroy(B->gstream[g]); }
  for (int g = 0; g < dmvio_hip_ba_batch::BA_BATCH_STREAMS; g++) for (int k = 0; k < 3; k++) if (B->gev[g][k]) hipEventDestroy(B->gev[g][k]);
  delete B;
}
// 1: the back substitution of the 68x68 solve in the host's order (one dependent chain of n^2 / 2 subtractions: x bit-identical to BAHost::ldltSolveTransposed, ~10 us more per
// iteration); 0 (default): column-oriented — the same terms in another association (measured |dx| <= 1e-12 relative, tests/test_ba_batch_gpu.py)
int dmvio_hip_ba_batch_set_exact_backsub(dmvio_hip_ba_batch* B, int on) {
  if (!B) return failmsg("ba_batch: null handle");
  std::lock_guard<std::mutex> lk(B->mu);
  B->exact_backsub = on ? 1 : 0;
  return 0;
}
int dmvio_hip_ba_batch_last_ms(dmvio_hip_ba_batch* B, float ms3[3]) {
  if (!B || !ms3) return failmsg("ba_batch: null argument");
  std::lock_guard<std::mutex> lk(B->mu);
  ms3[0] = B->last_ms[0]; ms3[1] = B->last_ms[1]; ms3[2] = B->last_ms[2];
  return 0;
}
// diagnostics: in-kernel timeline of window 0's last k_ba_solve of the last call, 100 MHz ticks since the kernel started: staged + settled, delta + bM_top + diagonal, system
// assembled, pivot order, permuted, factorised, back-substituted, x, resubstitution inputs + stepped states, exponentials, pair tables, energies
int dmvio_hip_ba_batch_last_solve_ticks(dmvio_hip_ba_batch* B, int ticks12[12]) {
  if (!B || !ticks12) return failmsg("ba_batch: null argument");
  std::lock_guard<std::mutex> lk(B->mu);
  for (int i = 0; i < 12; i++) ticks12[i] = B->h_wins[0].S.ticks[i];
  return 0;
}
// diagnostics: how window w's last k_ba_solve of the last call found its pivot order — 0 = ranks of the scaled diagonal (all |values| distinct), 1 = ties replayed
// (selection with swaps on one wavefront), 2 = a NaN on the diagonal (the literal loop)
int dmvio_hip_ba_batch_last_pivot_branch(dmvio_hip_ba_batch* B, int w, int* branch) {
  if (!B || !branch || w < 0 || w >= B->cap) return failmsg("ba_batch_last_pivot_branch: bad argument");
  std::lock_guard<std::mutex> lk(B->mu);
  *branch = B->h_wins[w].S.pivot_branch;
  return 0;
}
// Tests / diagnostics: the solve of EnergyFunctional.cpp:971-973 for a GIVEN system on the device, exactly as k_ba_solve runs it (Jacobi scaling (H_ii + 10)^-1/2, Eigen's
// pivot order, LDL^T, forward / back substitution on one 512-thread workgroup) — the device counterpart of dmvio_hip_ba_solve_ldlt.  HPassed: n x n row-major (the lower
// triangle is read), n = 4 + 8 F <= 100.  x_out[n]; perm_out[n] (may be NULL): the index the transpositions bring to position k; branch_out (may be NULL): 0 ranks /
// 1 ties / 2 NaN; zero_out (may be NULL): the matrix's first pivot was zero (x = 0).  exact_backsub as dmvio_hip_ba_batch_set_exact_backsub.
int dmvio_hip_ba_debug_solve(dmvio_hip_ctx* ctx, int n, const double* HPassed, const double* b_in, int exact_backsub, double* x_out, int* perm_out, int* branch_out, int* zero_out) {
  if (!ctx || !HPassed || !b_in || !x_out || n < 2 || n > 4 + 8 * BA_MAXF_CAP) return failmsg("ba_debug_solve: bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  double* d = nullptr;
  const size_t nin = (size_t)n * n + n, nout = 2 * (size_t)n + 2;
  HIPCHK(hipMalloc((void**)&d, sizeof(double) * (nin + nout)));
  std::vector<double> h(nin + nout, 0.0);
  memcpy(h.data(), HPassed, sizeof(double) * n * n); memcpy(h.data() + (size_t)n * n, b_in, sizeof(double) * n);
  hipError_t e = hipMemcpy(d, h.data(), sizeof(double) * nin, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const size_t lds = sizeof(double) * baSolveCoreLdsDoubles(n);
    BA_BY_MAXF((n + 3) / 8 /* the keyframes n unknowns stand for, rounded up */, M, hipLaunchKernelGGL((k_ba_solve_debug<M>), dim3(1), dim3(BA_SOLVE_THREADS), lds, nullptr, n, d, d + (size_t)n * n, exact_backsub, d + nin));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(h.data() + nin, d + nin, sizeof(double) * nout, hipMemcpyDeviceToHost);
  }
  hipFree(d);
  if (e != hipSuccess) return failmsg((std::string("ba_debug_solve: ") + hipGetErrorString(e)).c_str());
  const double* o = h.data() + nin;
  memcpy(x_out, o, sizeof(double) * n);
  if (perm_out) for (int i = 0; i < n; i++) perm_out[i] = (int)o[n + i];
  if (branch_out) *branch_out = (int)o[2 * n];
  if (zero_out) *zero_out = (int)o[2 * n + 1];
  return 0;
}
// 0 (default): a batch of >= 4 windows is cut into up to three groups on three streams (at least two windows each), their launches interleaved; k >= 1: at most k groups
// (1 = the whole batch on one stream).  The grouping changes no result: no arithmetic crosses windows.
int dmvio_hip_ba_batch_set_streams(dmvio_hip_ba_batch* B, int streams) {
  if (!B || streams < 0) return failmsg("ba_batch_set_streams: bad argument");
  std::lock_guard<std::mutex> lk(B->mu);
  B->streams = std::min<int>(streams, dmvio_hip_ba_batch::BA_BATCH_STREAMS);
  return 0;
}
// which linearisation kernel a batch of >= 4 windows runs: 1 (default) = k_ba_linearize_b1, one lane per residual; 8 = k_ba_linearize_b, eight lanes per residual (what a
// single window runs).  Same values either way.
int dmvio_hip_ba_batch_set_linearize_lanes(dmvio_hip_ba_batch* B, int lanes) {
  if (!B || (lanes != 1 && lanes != 8)) return failmsg("ba_batch_set_linearize_lanes: 1 or 8");
  std::lock_guard<std::mutex> lk(B->mu);
  B->lin_lanes = lanes;
  return 0;
}
// measurement: HIP events around the stepped linearisation of the second iteration (k_ba_linearize_b over all windows of the call) -> dmvio_hip_ba_batch_last_ms()[2]
int dmvio_hip_ba_batch_set_profile(dmvio_hip_ba_batch* B, int on) {
  if (!B) return failmsg("ba_batch: null handle");
  std::lock_guard<std::mutex> lk(B->mu);
  B->profile = on ? 1 : 0;
  return 0;
}
}  // extern "C"

// One call of the device-resident loop over Wn windows of equal keyframe count: the per-call state and the stages optimizeBatchGroup runs in order.
struct BatchCall {
  dmvio_hip_ba_batch* const B;
  const int Wn;
  dmvio_hip_ba* const* const hs;
  const int mnumOptIts;
  double* const x_last;   // Wn x BA_BATCH_NMAX or NULL: every window's last x
  const int F, n, F2;
  const BatchLayout L;    // this call's windows in the batch's slabs (B->slab: the strides)
  const hipStream_t s;
  const std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
  void stamp(const int k) { B->host_us[k] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_call).count(); }
  // the stream groups of the call (why and how they run: at optimizeBatchGroup)
  struct Grp { hipStream_t st; int w0, cnt; };
  int G = 1;
  Grp grp[dmvio_hip_ba_batch::BA_BATCH_STREAMS];
  int groupOf(const int w) const { int g = 0; while (g + 1 < G && w >= grp[g + 1].w0) g++; return g; }
  const BAWinDev* dwins(const Grp& q) const { return B->d_wins + q.w0; }
  // a group that holds a window with residuals kept linearised runs EnergyFunctional's three accumulations (L / A / Schur pass: accumulateLin in ba_loop_host.hpp) for those
  // windows; its other windows take their one ordinary accumulation in the A pass
  bool grpLin[dmvio_hip_ba_batch::BA_BATCH_STREAMS];
  // grid extents: the largest window's
  int gx_lin = 0, gx_pt8 = 0, gx_acc = 0, gx_res = 0, gx_pts = 0, gx_lin1 = 0;
  const int n_gather, n_stitch;
  const FrameStore fs;
  const size_t solveLds;
  // the eight-lane kernel hides latency (few windows); the one-lane kernel does an eighth of the lane work (a grid that fills the device)
  const bool lin1;
  const size_t patchLds = sizeof(float) * LIN_THREADS * BA_PATCH_STRIDE;   // the one-lane linearisation's per-lane 8x8 image windows
  // with workers the windows are prepared in index order behind the caller's back: group g + 1's while group g is enqueued
  std::atomic<int> prepared[dmvio_hip_ba_batch::BA_BATCH_STREAMS];
  std::atomic<int> prepare_failed{0};   // set BEFORE the window is counted: whoever sees a group complete (acquire) sees the failure of any of its windows
  bool async_prepare = false;
  enum { PREPARE_FAILED = 1 };          // enqueueInitial: a window's preparation failed (the workers hold the message); HIP errors are negative
  struct StreamSwap {   // the handles' own entry points (prepareWindow's table uploads) enqueue on the stream of the window's GROUP for the duration of the call: what a group's
                        // kernels read is then in front of them in stream order, whichever thread prepares the window and however late it does so
    std::vector<std::pair<dmvio_hip_ba*, hipStream_t>> saved;
    ~StreamSwap() { for (auto& kv : saved) kv.first->stream = kv.second; }
  } swap;
  struct WorkerWait {   // the workers run prepareWindow over this object: no way out of the call (HIPCHK returns) without waiting for them.  The LAST member: destroyed first,
                        // while everything the workers reference is still alive
    BAWorkers& wk; bool armed;
    ~WorkerWait() { if (armed) wk.waitAsync(false); }
  } workerWait;

  BatchCall(dmvio_hip_ba_batch* B_, const int Wn_, dmvio_hip_ba* const* hs_, const int its, double* x_last_)
      : B(B_), Wn(Wn_), hs(hs_), mnumOptIts(its), x_last(x_last_), F(hs_[0]->H.F), n(hs_[0]->H.n()), F2(F * F), L(n, F), s(B_->stream),
        n_gather((int)((L.outTrace() + 255) / 256)), n_stitch(F + F2), fs(B_->ctx->frames.built_and_waited()),
        solveLds(sizeof(double) * baSolveLdsDoubles(n, F, F <= BA_MAXF ? BASolveDims<BA_MAXF>::ALIAS_HM : BASolveDims<BA_MAXF_CAP>::ALIAS_HM)),
        lin1(B_->lin_lanes == 1 && Wn_ >= 4), workerWait{B_->workers, false} {
    const int maxG = B->streams > 0 ? B->streams : 3;   // measured (tools/ba_batch_streams.py): three groups are best at W = 16 and 64; a fourth stream shares a hardware queue
                                                          // with another one (GPU_MAX_HW_QUEUES = 4, one of them busy with the handles' own streams) and loses
    G = (Wn >= 4 && !B->profile) ? std::max(1, std::min(maxG, Wn / 2)) : 1;
    for (int g = 0; g < G; g++) {
      grp[g].st = B->gstream[g]; grp[g].w0 = (int)(((long long)Wn * g) / G); grp[g].cnt = (int)(((long long)Wn * (g + 1)) / G) - grp[g].w0;
      grpLin[g] = false;
      for (int w = grp[g].w0; w < grp[g].w0 + grp[g].cnt; w++) grpLin[g] = grpLin[g] || hs[w]->n_lin > 0;
      prepared[g].store(0, std::memory_order_relaxed);
    }
  }

  // ---- every window's stream becomes its group's (StreamSwap), and the grid extents of the call
  int handOverStreams() {
    for (int w = 0; w < Wn; w++) {
      dmvio_hip_ba* b = hs[w];
      const hipStream_t gs = grp[groupOf(w)].st;
      if (b->stream != gs) { HIPCHK(hipStreamSynchronize(b->stream)); swap.saved.emplace_back(b, b->stream); b->stream = gs; }
      gx_lin = std::max(gx_lin, b->n_lin_blocks); gx_pt8 = std::max(gx_pt8, b->n_pt8_blocks); gx_acc = std::max(gx_acc, b->accBlocks()); gx_res = std::max(gx_res, (b->H.R + 255) / 256); gx_pts = std::max(gx_pts, b->H.N);
    }
    gx_lin1 = (gx_res * 256 + LIN_THREADS - 1) / LIN_THREADS;
    stamp(0);
    if (!L.fitsIn(B->slab)) return failmsg("ba_optimize_batch: table slab too small");
    return 0;
  }

  // ---- the host side of one window before the loop: its record (BAWinDev) and its tables in the pinned slabs; the handle's own host-loop caches are given up
  int prepareWindow(const int w) {
    dmvio_hip_ba* b = hs[w];
    BAHost& H = b->H;
    b->deviceLoopTakes();
    if (int r = resolveTh(b)) return r;
    if (b->adj_dirty) { if (int r = uploadAdjoints(b)) return r; }   // on the group's stream (StreamSwap): in front of the group's first k_ba_stitch_b
    // (the precalc table, the thresholds and the activation of all residuals travel with the batch: one upload, one launch for all windows)
    H.getNullspaces();
    H.prepareOrthogonalize();
    // ---- the window's record
    BAWinDev& V = B->h_wins[w];
    memset(&V, 0, sizeof(V));
    fillWindow(b);
    V.W = b->W; V.Wb = b->W;
    V.P = b->P; V.Rs = b->Rs;
    V.D = makeDecide(b, 0, true, false);
    for (int f = 0; f < BA_MAXF_CAP; f++) V.frameTH[f] = f < F ? H.fr[f].frameEnergyTH : 0.0f;
    V.D.frameTH = B->d_wins[w].frameTH;   // (an address: the record's own copy on the device)
    dynFromHost(H, V.T); V.Tb = V.T;
    b->dyn_cur = V.T;
    V.A = b->accumArgs();
    V.SB = b->SB; V.adHost = b->d_adHost; V.adTarget = b->d_adTarget;
    V.ctl = b->d_ctl;
    V.n_lin_blocks = b->n_lin_blocks; V.n_pt8_blocks = b->n_pt8_blocks; V.n_acc_blocks = b->accBlocks();
    V.n_res_blocks = (H.R + 255) / 256; V.n_gather_blocks = n_gather; V.n_stitch_blocks = n_stitch; V.n_lin1_blocks = (H.R + LIN_THREADS - 1) / LIN_THREADS;
    BASolveDev& S = V.S;
    S.F = F; S.n = n; S.stepped = 0; S.iterations_done = 0; S.n_accepted = 0; S.exact_backsub = B->exact_backsub;
    S.lambda = 1e-5;
    S.lastL = calcLEnergy(b); S.lastM = H.calcMEnergy(); S.newL = S.lastL; S.newM = S.lastM;
    // residuals kept linearised (dmvio_hip_ba_fix_linearization): what the three-pass accumulation and the linearised energy read, at the deltas of the state the window enters with
    V.n_lin = b->n_lin; V.n_lin_runs = (H.N + 49) / 50; V.lin_cnt = 0;
    if (b->n_lin > 0) {
      V.fullJ = b->d_fullJ; V.lin = b->d_lin; V.rtz = b->d_rtz; V.linRec = b->d_linRec; V.linActive = b->d_linActive; V.topActive = b->d_topActive; V.linE = b->d_linE;
      std::vector<float> adHT;
      H.adHTdeltaF(adHT);
      for (int k = 0; k < 2; k++) { memcpy(V.adHTdelta[k], adHT.data(), sizeof(float) * adHT.size()); for (int i = 0; i < 4; i++) V.cDeltaF[k][i] = H.cDeltaF[i]; }
    }
    for (int i = 0; i < 4; i++) { S.c_value[i] = H.c_value[i]; S.c_value_zero[i] = H.c_value_zero[i]; S.c_value_backup[i] = H.c_value[i]; S.cPrior[i] = H.cPrior[i]; S.cPriorF[i] = H.cPriorF[i]; }
    for (int f = 0; f < F; f++) {
      BAFrameDev& q = S.fr[f]; const BAFrameHost& h = H.fr[f];
      q.evalPT = h.evalPT; q.ab_exposure = h.ab_exposure;
      for (int i = 0; i < 10; i++) { q.state[i] = h.state[i]; q.state_zero[i] = h.state_zero[i]; q.state_backup[i] = h.state[i]; }
      for (int i = 0; i < 8; i++) q.prior[i] = h.prior[i];
    }
    // ---- the uploaded tables (BatchLayout): filled in the pinned slab, addressed in the device slab
    char* tab = B->hTab(w);
    const char* dtab = B->dTab(w);
    const bool haveM = H.HM.size() == (size_t)n * n;
    S.haveM = haveM ? 1 : 0;
    if (haveM) { memcpy(tab + L.tabHM(), H.HM.data(), sizeof(double) * n * n); memcpy(tab + L.tabBM(), H.bM.data(), sizeof(double) * n); }
    S.nBasis = (int)H.orthoBasis.size();
    for (int k = 0; k < S.nBasis; k++) memcpy(tab + L.tabBasis() + sizeof(double) * k * n, H.orthoBasis[k].data(), sizeof(double) * n);
    memcpy(tab + L.tabAdHostF(), H.adHostF.data(), L.tabAdBytes()); memcpy(tab + L.tabAdTargetF(), H.adTargetF.data(), L.tabAdBytes());
    memcpy(tab + L.tabPre(), H.pre.data(), L.tabPreBytes());
    S.HM = reinterpret_cast<const double*>(dtab + L.tabHM()); S.bM = reinterpret_cast<const double*>(dtab + L.tabBM()); S.basis = reinterpret_cast<const double*>(dtab + L.tabBasis());
    S.adHostF = reinterpret_cast<const float*>(dtab + L.tabAdHostF()); S.adTargetF = reinterpret_cast<const float*>(dtab + L.tabAdTargetF());
    V.pre = reinterpret_cast<const BAPrecalc*>(dtab + L.tabPre());
    // ---- the device output: [sys | resInA | trace | x_last | sysL]
    double* out = B->dOut(w);
    V.sys = out;
    S.trace = out + L.outTrace(); S.x_last = out + L.outXLast();
    V.sysL = out + L.outSysL();
    return 0;
  }
  // all windows: on the workers behind the caller's back where that pays (enqueueInitial waits group by group), else here and now
  int prepareWindows() {
    async_prepare = !B->workers.th.empty() && Wn >= 8 && G > 1;
    if (!async_prepare) return B->workers.parallelFor(Wn, [this](const int w) { return prepareWindow(w); });
    B->workers.startAsync(Wn, [this](const int w) -> int {
      const int r = prepareWindow(w);
      if (r) prepare_failed.store(1, std::memory_order_relaxed);
      prepared[groupOf(w)].fetch_add(1, std::memory_order_release);
      return r;
    });
    workerWait.armed = true;
    return 0;
  }
  // the workers are done (or never ran): their error, or -1 for a launch loop that stopped at a failed window, with every stream of the call drained
  int joinPrepare(const bool launched) {
    if (!async_prepare) return 0;
    workerWait.armed = false;
    const int r = B->workers.waitAsync();
    if (r || !launched) { for (int g = 0; g < G; g++) hipStreamSynchronize(grp[g].st); return r ? r : -1; }
    return 0;
  }

  // ---- launches shared by the stages
  void linearize(const Grp& q, const int kind) {
    if (lin1) hipLaunchKernelGGL(k_ba_linearize_b1, dim3(gx_lin1, q.cnt), dim3(LIN_THREADS), patchLds, q.st, dwins(q), fs, kind);
    else hipLaunchKernelGGL(k_ba_linearize_b, dim3(gx_lin, q.cnt), dim3(LIN_THREADS), 0, q.st, dwins(q), fs, kind);
  }
  void solve(const Grp& q, const int it, const bool finish) {
    if (finish) BA_BY_MAXF(F, M, hipLaunchKernelGGL((k_ba_solve<M, true>), dim3(q.cnt), dim3(BA_SOLVE_THREADS), solveLds, q.st, B->d_wins + q.w0, it));
    else BA_BY_MAXF(F, M, hipLaunchKernelGGL((k_ba_solve<M, false>), dim3(q.cnt), dim3(BA_SOLVE_THREADS), solveLds, q.st, B->d_wins + q.w0, it));
  }
  void linRecords(const Grp& q, const int gate, const bool sums) {   // the addPoint<1> records (and the A / L activity views); sums: + the linearised residuals' per-point sums
    hipLaunchKernelGGL(k_ba_lin_records_b, dim3(gx_res, q.cnt), dim3(256), 0, q.st, dwins(q), gate);
    if (sums) hipLaunchKernelGGL(k_ba_lin_point_sums_b, dim3((gx_pts + 255) / 256, q.cnt), dim3(256), 0, q.st, dwins(q), gate);
  }
  void chain(const int g, const int backup, const int apply, const int gate, const bool sums_done) {   // applyRes + per-point sums -> accumulate -> stitch -> gather: the system of the (new) state
    const Grp& q = grp[g];
    const BAWinDev* dwq = dwins(q);
    if (!sums_done) hipLaunchKernelGGL(k_ba_point_sums_b, dim3(gx_pt8, q.cnt), dim3(256), 0, q.st, dwq, backup, apply, gate);
    for (int pass = grpLin[g] ? (int)BA_PASS_L : (int)BA_PASS_ALL; pass <= (grpLin[g] ? (int)BA_PASS_S : (int)BA_PASS_ALL); pass++) {
      hipLaunchKernelGGL(k_ba_accumulate_b, dim3(gx_acc, q.cnt), dim3(256), 0, q.st, dwq, gate, pass);
      hipLaunchKernelGGL(k_ba_stitch_b, dim3(n_stitch, q.cnt), dim3(64 * F), sizeof(StitchWave) * F, q.st, dwq, gate, pass);
      BA_BY_MAXF(F, M, hipLaunchKernelGGL((k_ba_stitch_gather_b<M>), dim3(n_gather, q.cnt), dim3(256), 0, q.st, dwq, gate, pass));
    }
  }

  // ---- group g: its windows' tables (prepared by now) and records go up, then every residual still in the graph active again (FullSystemOptimize.cpp:431-448), initial
  // linearisation, applyRes and the first system (:450-470)
  int enqueueInitial(const int g) {
    const Grp& q = grp[g];
    const BAWinDev* dwq = dwins(q);
    if (async_prepare) while (prepared[g].load(std::memory_order_acquire) < q.cnt) __builtin_ia32_pause();
    if (g == 0) stamp(1);
    if (async_prepare && prepare_failed.load(std::memory_order_relaxed)) return PREPARE_FAILED;   // nothing of the failed window (or of the groups behind it) is launched
    if (g == 0) { HIPCHK(hipEventRecord(B->ev[0], s)); for (int k = 1; k < G; k++) HIPCHK(hipStreamWaitEvent(grp[k].st, B->ev[0], 0)); }   // (the other streams: behind whatever the batch's stream still holds; prepareWindow's own uploads need no event: they are on the group's stream)
    HIPCHK(hipMemcpyAsync(B->d_wins + q.w0, B->h_wins + q.w0, sizeof(BAWinDev) * q.cnt, hipMemcpyHostToDevice, q.st));
    HIPCHK(hipMemcpyAsync(B->dTab(q.w0), B->hTab(q.w0), B->slab.tabStride() * (size_t)(q.cnt - 1) + L.tabUsed(), hipMemcpyHostToDevice, q.st));
    if (g > 0) HIPCHK(hipStreamWaitEvent(q.st, B->gev[g - 1][0], 0));   // the stagger
    hipLaunchKernelGGL(k_ba_reset_oob_b, dim3(gx_res, q.cnt), dim3(256), 0, q.st, dwq);
    linearize(q, BA_LINB_INITIAL);
    if (g + 1 < G) HIPCHK(hipEventRecord(B->gev[g][0], q.st));
    hipLaunchKernelGGL(k_ba_apply_b, dim3(gx_res, q.cnt), dim3(256), 0, q.st, dwq, 0, (int)BA_GATE_ALWAYS);
    if (grpLin[g]) linRecords(q, BA_GATE_ALWAYS, true);
    chain(g, 1, 0, BA_GATE_ALWAYS, false);
    return 0;
  }
  // ---- one iteration of the loop (:485-586) for group g: nothing in it waits for the host
  int enqueueIteration(const int g, const int it) {
    const Grp& q = grp[g];
    const BAWinDev* dwq = dwins(q);
    solve(q, it, false);
    if (grpLin[g]) hipLaunchKernelGGL(k_ba_lin_energy_b, dim3(gx_res, q.cnt), dim3(256), 0, q.st, B->d_wins + q.w0);   // E_L's linearised term of the stepped state, for the accept test
    const bool prof = B->profile && g == 0 && it == std::min(1, mnumOptIts - 1);
    if (prof) HIPCHK(hipEventRecord(B->ev[4], q.st));
    if (lin1) { hipLaunchKernelGGL(k_ba_resubstitute_b, dim3(gx_pt8, q.cnt), dim3(256), 0, q.st, dwq); linearize(q, BA_LINB_STEPPED_DONE); }
    else linearize(q, BA_LINB_STEPPED);
    if (prof) HIPCHK(hipEventRecord(B->ev[5], q.st));
    // rejected: restore + relinearise | accepted: applyRes + per-point sums (the last iteration's accepted step is only applied: nobody solves its system) — one launch
    const int what = it < mnumOptIts - 1 ? 0 : 1;
    if (grpLin[g] && what == 0) linRecords(q, BA_GATE_ACCEPTED, true);   // (the per-point sums below add the linearised residuals' Hdd / bd / Hcd)
    const int gx_post = std::max(lin1 ? gx_lin1 : gx_lin, what == 0 ? gx_pt8 : gx_res);
    if (lin1) hipLaunchKernelGGL((k_ba_post_decide_b<true>), dim3(gx_post, q.cnt), dim3(LIN_THREADS), patchLds, q.st, dwq, fs, what);
    else hipLaunchKernelGGL((k_ba_post_decide_b<false>), dim3(gx_post, q.cnt), dim3(LIN_THREADS), 0, q.st, dwq, fs, what);
    if (grpLin[g] && what == 0) linRecords(q, BA_GATE_ACCEPTED, false);  // (again behind applyRes: the A pass's activity view follows the applied states)
    if (what == 0) chain(g, 1, 1, BA_GATE_ACCEPTED, true);
    return 0;
  }
  // ---- settle the last decision; the group's states and traces come back on its own stream: [resInA | trace (64 x 4) | x_last] of a window is the tail of its system
  // slab, one strided copy per group
  int enqueueSettle(const int g) {
    const Grp& q = grp[g];
    solve(q, mnumOptIts, true);
    HIPCHK(hipMemcpyAsync(B->h_wins + q.w0, B->d_wins + q.w0, sizeof(BAWinDev) * q.cnt, hipMemcpyDeviceToHost, q.st));
    HIPCHK(hipMemcpy2DAsync(B->hMirror(q.w0), sizeof(double) * BatchLayout::MIRROR_STRIDE, B->dOut(q.w0) + L.outResInA(), B->slab.outStride(), sizeof(double) * L.mirrorUsed(), q.cnt,
                            hipMemcpyDeviceToHost, q.st));
    HIPCHK(hipEventRecord(B->gev[g][1], q.st));
    return 0;
  }

  // ---- back on the host: a window's optimised states, then the newest keyframe's new evaluation point (:596-603) in the handle, the record and the pinned pair table
  int writeBackWindow(const int w) {
    dmvio_hip_ba* b = hs[w];
    BAHost& H = b->H;
    BAWinDev& V = B->h_wins[w];
    const BASolveDev& S = V.S;
    H.calibSetValue(S.c_value);
    for (int i = 0; i < 4; i++) H.c_value_backup[i] = S.c_value_backup[i];
    for (int f = 0; f < F; f++) {
      BAHost::frameSetState(H.fr[f], S.fr[f].state);
      for (int i = 0; i < 10; i++) H.fr[f].state_backup[i] = S.fr[f].state_backup[i];
    }
    const double* m = B->hMirror(w);
    const double* tr = m + BatchLayout::MIRROR_TRACE;
    const double* xl = m + BatchLayout::MIRROR_XLAST;
    H.resInA = (int)m[0];   // the count the last accumulation left behind (ef->resInA after the loop)
    const int done = S.iterations_done;
    b->iterations_done = done;
    for (int k = 0; k <= done && k < 64; k++) for (int c = 0; c < 4; c++) b->trace[k][c] = tr[4 * k + c];   // row 0: the initial state (written by the first solve)
    b->H.lastX.assign(xl, xl + n);
    if (x_last) memcpy(x_last + (size_t)BA_BATCH_NMAX * w, xl, sizeof(double) * n);
    H.reanchorNewest();
    memcpy(B->hTab(w) + L.tabPre(), H.pre.data(), L.tabPreBytes());
    fillWindow(b);
    V.W = b->W;
    dynFromHost(H, V.T);
    b->deviceLoopReturns(V.T);
    return 0;
  }
  // wait for group g's states and write them back (the workers share a group's windows)
  int writeBackGroup(const int g) {
    const Grp& q = grp[g];
    HIPCHK(hipEventSynchronize(B->gev[g][1]));
    if (g == 0) stamp(3);
    if (int r = B->workers.parallelFor(q.cnt, [&](const int i) { return writeBackWindow(q.w0 + i); }, 4)) { for (int k = 0; k < G; k++) hipStreamSynchronize(grp[k].st); return r; }
    if (g == G - 1) stamp(4);
    return 0;
  }
  // ---- upload group g's re-anchored records / pair tables and enqueue its final fix-linearisation (:604-609) on its stream
  int enqueueFinal(const int g) {
    const Grp& q = grp[g];
    HIPCHK(hipMemcpyAsync(B->d_wins + q.w0, B->h_wins + q.w0, sizeof(BAWinDev) * q.cnt, hipMemcpyHostToDevice, q.st));
    HIPCHK(hipMemcpy2DAsync(B->dTab(q.w0) + L.tabPre(), B->slab.tabStride(), B->hTab(q.w0) + L.tabPre(), B->slab.tabStride(), L.tabPreBytes(), q.cnt,
                            hipMemcpyHostToDevice, q.st));   // the re-anchored pair tables
    if (g == 0) HIPCHK(hipEventRecord(B->ev[2], q.st));
    linearize(q, BA_LINB_FINAL);
    hipLaunchKernelGGL(k_ba_apply_b, dim3(gx_res, q.cnt), dim3(256), 0, q.st, B->d_wins + q.w0, 1, (int)BA_GATE_ALWAYS);   // applyRes + linearizeAll(true)'s removal of inactive residuals
    HIPCHK(hipGetLastError());
    if (g > 0) { HIPCHK(hipEventRecord(B->gev[g][2], q.st)); HIPCHK(hipStreamWaitEvent(s, B->gev[g][2], 0)); }
    return 0;
  }
  // ---- the second wait, the call's device times and every window's results
  int collect(float* rmse, double* finalEnergy, int* iterations, double* trace) {
    HIPCHK(hipEventRecord(B->ev[3], s));
    stamp(5);
    HIPCHK(hipStreamSynchronize(s));
    stamp(6);
    // HIP-event times: [0] the whole call on the device (first upload .. last kernel), [1] from the first group's final linearisation to the last kernel
    HIPCHK(hipEventElapsedTime(&B->last_ms[0], B->ev[0], B->ev[3]));
    HIPCHK(hipEventElapsedTime(&B->last_ms[1], B->ev[2], B->ev[3]));
    B->last_ms[0] -= B->last_ms[1];   // (callers add the two)
    B->last_ms[2] = 0;
    if (B->profile) HIPCHK(hipEventElapsedTime(&B->last_ms[2], B->ev[4], B->ev[5]));
    for (int w = 0; w < Wn; w++) {
      dmvio_hip_ba* b = hs[w];
      BAHost& H = b->H;
      if (b->n_lin > 0) {   // accumulateLF_MT's system of the last accumulation, for dmvio_hip_ba_get_lf_system and the host-side solve entry points
        std::vector<double> lf(L.sysLDoubles());
        HIPCHK(hipMemcpy(lf.data(), B->h_wins[w].sysL, sizeof(double) * lf.size(), hipMemcpyDeviceToHost));
        H.HLraw.assign(lf.begin(), lf.begin() + (size_t)n * n); H.bLraw.assign(lf.begin() + (size_t)n * n, lf.end());
      }
      const double fe = b->h_res->E[0];
      H.fr[F - 1].frameEnergyTH = b->h_res->th[0];
      b->final_energy = fe;
      if (rmse) rmse[w] = sqrtf((float)(fe / (8 * H.resInA)));
      if (finalEnergy) finalEnergy[w] = fe;
      if (iterations) iterations[w] = b->iterations_done;
      if (trace) memcpy(trace + (size_t)BatchLayout::TRACE * w, b->trace, sizeof(b->trace));
      // the staging area of this call's uploads is free again: they went out on the group's stream in front of the group's last kernel, which `s` has waited for (gev[g][2])
      // before the host waited for `s` above — so waiting for `s` covers them (and costs nothing more: a first host wait on each group's stream measured ~2 % of a W = 16 call)
      if (b->bounce.used || !b->bounce.outs.empty()) HIPCHK(b->bounce.finish(s));
    }
    stamp(7);
    return 0;
  }
};

// Up to three groups of windows by default (at most BA_BATCH_STREAMS on request), one stream each, from 4 windows on: k_ba_solve is one workgroup per window (a 50 us latency chain on a handful of CUs), so while one
// group solves, the other groups' linearisations / accumulations fill the device.  The groups share nothing.  Their launches are enqueued STAGE BY STAGE (initial chain of
// every group, iteration 0 of every group, ...): a stream whose commands the host has not submitted yet cannot overlap with anything (measured: with the groups enqueued one
// after the other the second one started three iterations late).  Group g starts behind group g-1's initial linearisation, which keeps the groups out of step.  A profiled
// call (dmvio_hip_ba_batch_set_profile) runs as ONE group: its timed linearisation then covers all windows of the call, alone on the device.
// The host's per-window work is pipelined along the groups too: group g's tables are prepared, uploaded and its first chain enqueued while the device already works on the
// groups before it; behind the loop group g's states are written back (and its final linearisation enqueued) while the later groups still run their last iterations.
static int optimizeBatchGroup(dmvio_hip_ba_batch* B, const int Wn, dmvio_hip_ba* const* hs, int mnumOptIts, float* rmse, double* finalEnergy, int* iterations, double* trace,
                              double* x_last) {
  const int F = hs[0]->H.F;
  if (F < 2) { for (int w = 0; w < Wn; w++) { if (rmse) rmse[w] = 0; if (iterations) iterations[w] = 0; if (finalEnergy) finalEnergy[w] = 0; } return 0; }
  mnumOptIts = BAHost::optIterations(F, mnumOptIts);
  if (mnumOptIts < 1) return failmsg("ba_optimize_batch: mnumOptIts < 1 (the device-resident loop writes the trace's first row in its first solve)");
  BatchCall c(B, Wn, hs, mnumOptIts, x_last);
  if (int r = c.handOverStreams()) return r;
  if (int r = c.prepareWindows()) return r;
  bool launched = true;
  for (int g = 0; g < c.G && launched; g++) {
    const int r = c.enqueueInitial(g);
    if (r < 0) return r;
    launched = r != BatchCall::PREPARE_FAILED;
  }
  if (int r = c.joinPrepare(launched)) return r;
  for (int it = 0; it < mnumOptIts; it++)
    for (int g = 0; g < c.G; g++) if (int r = c.enqueueIteration(g, it)) return r;
  for (int g = 0; g < c.G; g++) if (int r = c.enqueueSettle(g)) return r;
  HIPCHK(hipGetLastError());
  c.stamp(2);
  // group by group, in the order they finish (the stagger)
  for (int g = 0; g < c.G; g++) {
    if (int r = c.writeBackGroup(g)) return r;
    if (int r = c.enqueueFinal(g)) return r;
  }
  return c.collect(rmse, finalEnergy, iterations, trace);
}

// ================================================================================================= point marginalisation, W windows per call
// dmvio_hip_ba_marginalize_points (capi_ba.hip) for W windows: FullSystem::flagPointsForRemoval's relinearisation (FullSystem.cpp:829-859) + marginalizePointsF
// (EnergyFunctional.cpp:678-742).  The windows are ordered by keyframe count (the stitch kernels want one F per launch; the caller's order inside a count), every window's
// record, pair table, candidates and — where the device copy is stale — adjoints are filled in the pinned slabs and go up in three copies; per count six launches
// (ba_batch_kernels.hpp); the systems and decisions come back in one copy behind one wait; then the host tail of the single call per window.  What the single call does to
// the handle beyond its results is done here too (the window's kernel arguments refreshed, the isLinearized bookkeeping of FullSystem.cpp:840-843); what it merely
// refreshes on the device (the handle's own pair table, threshold and adjoint copies) keeps its dirty flag instead and is refreshed by the next single call that needs it.
struct MargBatchCall {
  dmvio_hip_ba_batch* const B;
  const int W;
  dmvio_hip_ba_marg_window* const win;
  std::vector<int> order;                    // record k holds window order[k]
  struct Grp { int w0, cnt, F; };
  std::vector<Grp> grp;
  std::vector<size_t> candOff, outOff;       // per record, into the marginalisation buffer
  size_t inBytes = 0, outBytes = 0;        // [candidates of every window | per window its systems, resInA and decisions]: the first part goes up, the second comes back
  bool anyAdjoints = false;
  MargBatchCall(dmvio_hip_ba_batch* B_, const int W_, dmvio_hip_ba_marg_window* win_) : B(B_), W(W_), win(win_) {}

  int plan() {
    std::vector<char> done(W, 0);
    for (int i = 0; i < W; i++) {
      if (done[i]) continue;
      Grp g{(int)order.size(), 0, win[i].ba->H.F};
      for (int j = i; j < W; j++) if (!done[j] && win[j].ba->H.F == g.F) { order.push_back(j); done[j] = 1; g.cnt++; }
      grp.push_back(g);
    }
    candOff.resize(W); outOff.resize(W);
    DmvCursor C;
    for (int k = 0; k < W; k++) candOff[k] = C.takeBytes((size_t)win[order[k]].ba->H.N);
    inBytes = C.bytes();
    for (int k = 0; k < W; k++) {
      const dmvio_hip_ba* b = win[order[k]].ba;
      const BatchLayout L(b->H.n(), b->H.F);
      if (!L.margFitsIn(B->slab)) return failmsg("ba_marginalize_points_batch: table slab too small");
      outOff[k] = C.takeBytes(L.margOutDecision() + (size_t)b->H.N);
      anyAdjoints = anyAdjoints || b->adj_dirty;
    }
    outBytes = C.bytes() - inBytes;
    return B->margBegin(C.bytes(), &B->marg_work);
  }

  // ---- the host side of record k before the launches: the handle's part of the single call, the window's record and its tables in the pinned slabs
  int prepareWindow(const int k) {
    dmvio_hip_ba_marg_window& q = win[order[k]];
    dmvio_hip_ba* b = q.ba;
    BAHost& H = b->H;
    const int F = H.F, F2 = F * F, N = H.N, R = H.R;
    const BatchLayout L(H.n(), F);
    b->stateChanged();
    if (int r = resolveTh(b)) return r;
    fillWindow(b);
    BAWinDev& V = B->h_wins[k];
    memset(&V, 0, sizeof(V));
    V.W = b->W; V.Wb = b->W;
    V.D = makeDecide(b, -1, false, false);   // masked relinearisation: no energy / threshold / accept pass
    for (int f = 0; f < BA_MAXF_CAP; f++) V.frameTH[f] = f < F ? H.fr[f].frameEnergyTH : 0.0f;
    V.D.frameTH = B->d_wins[k].frameTH;
    // FullSystem.cpp:840-843: a candidate point's residuals are relinearised with isLinearized = false (the device clears its flags in k_ba_marg_apply_fix_b; the masked
    // kernels in front of it do not read them)
    if (b->n_lin > 0) {
      V.margLinClear = b->d_lin;
      for (int ri = 0; ri < R; ri++) if (q.candidates[b->h_point[ri]] && b->h_lin[ri]) { b->h_lin[ri] = 0; b->n_lin--; }
      b->n_lin_global = b->n_lin;
      if (b->n_lin == 0) { b->Rs.lin = nullptr; b->P.lHdd = b->P.lbd = b->P.lHcd = nullptr; b->P.HcdAF = nullptr; b->H.HLraw.clear(); b->H.bLraw.clear(); }
    }
    V.P = b->P; V.Rs = b->Rs;
    V.A = b->accumArgs();
    V.SB = b->SB; V.ctl = b->d_ctl;
    V.n_lin_blocks = b->n_lin_blocks; V.n_pt8_blocks = b->n_pt8_blocks; V.n_pt_blocks = b->n_pt_blocks; V.n_acc_blocks = b->accBlocks();
    V.n_res_blocks = (R + 255) / 256; V.n_gather_blocks = (int)((L.margSysDoubles() + 255) / 256); V.n_stitch_blocks = F + F2; V.n_lin1_blocks = (R + LIN_THREADS - 1) / LIN_THREADS;
    // deltas at the current state (EnergyFunctional::setDeltaF, EnergyFunctional.cpp:175-198)
    std::vector<float> adHT;
    H.adHTdeltaF(adHT);
    memcpy(V.adHTdelta[0], adHT.data(), sizeof(float) * adHT.size());
    for (int i = 0; i < 4; i++) V.cDeltaF[0][i] = H.cDeltaF[i];
    // the uploaded tables: the pair table of the current state; the adjoints where the handle's device copy is stale (it stays stale: adj_dirty is kept)
    char* tab = B->hTab(k);
    char* dtab = B->dTab(k);
    memcpy(tab + L.margTabPre(), H.pre.data(), L.tabPreBytes());
    V.pre = reinterpret_cast<const BAPrecalc*>(dtab + L.margTabPre());
    if (b->adj_dirty) {
      memcpy(tab + L.margTabAdHost(), H.adHost.data(), L.margTabAdBytes()); memcpy(tab + L.margTabAdTarget(), H.adTarget.data(), L.margTabAdBytes());
      V.adHost = reinterpret_cast<const double*>(dtab + L.margTabAdHost()); V.adTarget = reinterpret_cast<const double*>(dtab + L.margTabAdTarget());
    } else { V.adHost = b->d_adHost; V.adTarget = b->d_adTarget; }
    const auto cand = B->marg.put<unsigned char>(candOff[k]);
    memcpy(cand.h, q.candidates, (size_t)N); V.margCand = cand.d;
    V.margSys = B->marg.dev<double>(outOff[k]);
    V.margDecision = B->marg.dev<unsigned char>(outOff[k] + L.margOutDecision());
    V.margFullJ = b->d_fullJ; V.margRec = b->d_margRec; V.margActive = b->d_margActive;
    V.mHdiF = b->d_mHdiF; V.mbdSumF = b->d_mbdSumF; V.mHcd = b->d_mHcd;
    return 0;
  }

  int enqueue() {
    const hipStream_t s = B->stream;
    DmvWork& work = B->marg_work;
    // a handle's own stream may still hold work (its entry points return on a ticket, not on an empty stream): in front of the call
    for (int k = 0; k < W; k++) {
      dmvio_hip_ba* b = win[order[k]].ba;
      if (b->stream == s || hipStreamQuery(b->stream) == hipSuccess) continue;
      HIPCHK(hipEventRecord(B->marg_ev, b->stream));
      HIPCHK(hipStreamWaitEvent(s, B->marg_ev, 0));
    }
    (void)hipGetLastError();   // (hipErrorNotReady of the query above is no error)
    if (B->profile) HIPCHK(hipEventRecord(B->ev[6], s));
    HIPCHK(hipMemcpyAsync(B->d_wins, B->h_wins, sizeof(BAWinDev) * W, hipMemcpyHostToDevice, s)); work.uploads++;
    size_t tabWidth = 0;
    for (const Grp& g : grp) tabWidth = std::max(tabWidth, BatchLayout(4 + 8 * g.F, g.F).margTabUsed(anyAdjoints));
    HIPCHK(hipMemcpy2DAsync(B->dTab(0), B->slab.tabStride(), B->hTab(0), B->slab.tabStride(), tabWidth, W, hipMemcpyHostToDevice, s)); work.uploads++;
    if (int r = B->marg.upload(s, inBytes)) return r;
    const FrameStore fs = B->ctx->frames.built_and_waited();
    for (const Grp& g : grp) {
      int gx_lin = 0, gx_res = 0, gx_pt = 0, gx_acc = 0;
      for (int k = g.w0; k < g.w0 + g.cnt; k++) {
        const BAWinDev& V = B->h_wins[k];
        gx_lin = std::max(gx_lin, V.n_lin_blocks); gx_res = std::max(gx_res, V.n_res_blocks); gx_pt = std::max(gx_pt, V.n_pt_blocks); gx_acc = std::max(gx_acc, V.n_acc_blocks);
      }
      const BAWinDev* dw = B->d_wins + g.w0;
      const int F = g.F, n_gather = B->h_wins[g.w0].n_gather_blocks;
      hipLaunchKernelGGL(k_ba_marg_linearize_b, dim3(gx_lin, g.cnt), dim3(LIN_THREADS), 0, s, dw, fs); work.launches++;
      hipLaunchKernelGGL(k_ba_marg_apply_fix_b, dim3(gx_res, g.cnt), dim3(256), 0, s, dw); work.launches++;
      hipLaunchKernelGGL(k_ba_marg_point_sums_b, dim3(gx_pt, g.cnt), dim3(256), 0, s, dw); work.launches++;
      hipLaunchKernelGGL(k_ba_accumulate_bm, dim3(gx_acc, g.cnt), dim3(256), 0, s, dw); work.launches++;
      hipLaunchKernelGGL(k_ba_stitch_b, dim3(F + F * F, g.cnt), dim3(64 * F), sizeof(StitchWave) * F, s, dw, (int)BA_GATE_ALWAYS, (int)BA_PASS_M); work.launches++;
      BA_BY_MAXF(F, M, hipLaunchKernelGGL((k_ba_stitch_gather_b<M>), dim3(n_gather, g.cnt), dim3(256), 0, s, dw, (int)BA_GATE_ALWAYS, (int)BA_PASS_M)); work.launches++;
      HIPCHK(hipGetLastError());
    }
    if (int r = B->marg.download(s, inBytes, outBytes)) return r;
    if (B->profile) HIPCHK(hipEventRecord(B->ev[7], s));
    if (int r = B->marg.wait(s)) return r;
    B->marg_ms = 0;
    if (B->profile) HIPCHK(hipEventElapsedTime(&B->marg_ms, B->ev[6], B->ev[7]));
    return 0;
  }

  // ---- behind the wait: the host tail of the single call (the increment 0.25 (M - Msc) of HM / bM, the prior, the residual count; ef->resInA stays what it was)
  int finishWindow(const int k) {
    dmvio_hip_ba_marg_window& q = win[order[k]];
    BAHost& H = q.ba->H;
    const int n = H.n(), N = H.N;
    const BatchLayout L(n, H.F);
    const double* M = B->marg.host<const double>(outOff[k]);
    const double* Mb = M + (size_t)n * n; const double* Msc = Mb + n; const double* Mbsc = Msc + (size_t)n * n;
    if (H.HM.size() != (size_t)n * n) { H.HM.assign((size_t)n * n, 0.0); H.bM.assign(n, 0.0); }
    for (size_t i = 0; i < (size_t)n * n; i++) { const double v = BA_MARG_WEIGHT_FAC * (M[i] - Msc[i]); if (q.Hadd) q.Hadd[i] = v; if (q.update_prior) H.HM[i] += v; }
    for (int i = 0; i < n; i++) { const double v = BA_MARG_WEIGHT_FAC * (Mb[i] - Mbsc[i]); if (q.badd) q.badd[i] = v; if (q.update_prior) H.bM[i] += v; }
    q.resInM = (int)M[L.outResInA()];
    memcpy(q.decision, B->marg.host<char>(outOff[k] + L.margOutDecision()), (size_t)N);
    return 0;
  }
};

#include "ba_marg_frame_host.hpp"   // dmvio_hip_ba_marginalize_frame_batch and its two accessors

extern "C" {
int dmvio_hip_ba_marginalize_points_batch(dmvio_hip_ba_batch* B, int W, dmvio_hip_ba_marg_window* win) {
  if (!B) return failmsg("ba_marginalize_points_batch: null batch");
  if (W < 0) return failmsg("ba_marginalize_points_batch: W < 0");
  if (W > B->cap) return failmsg("ba_marginalize_points_batch: more windows than the batch was created for");
  std::lock_guard<std::mutex> lkB(B->mu);
  B->marg_work.clear();
  if (W == 0) return 0;
  if (!win) return failmsg("ba_marginalize_points_batch: null window list");
  std::vector<dmvio_hip_ba*> order(W);
  for (int i = 0; i < W; i++) {
    if (!win[i].ba) return failmsg("ba_marginalize_points_batch: null window");
    if (!win[i].candidates || !win[i].decision) return failmsg("ba_marginalize_points_batch: null candidates / decision");
    if (win[i].ba->ctx != B->ctx) return failmsg("ba_marginalize_points_batch: a window belongs to another context");
    order[i] = win[i].ba;
  }
  // the handles' locks, in address order (as dmvio_hip_ba_optimize_batch)
  if (dmvFirstRepeated(win, W, &dmvio_hip_ba_marg_window::ba) >= 0) return failmsg("ba_marginalize_points_batch: a window appears twice");
  std::sort(order.begin(), order.end());
  std::vector<std::unique_lock<std::recursive_mutex>> locks;
  for (dmvio_hip_ba* b : order) locks.emplace_back(b->mu);
  for (int i = 0; i < W; i++) {
    if (!win[i].ba->graph_ready) return failmsg("ba_marginalize_points_batch: window / graph not set");
    if (sharded(win[i].ba)) return failmsg("ba_marginalize_points_batch: a window sharded over ranks cannot join a batch");
  }
  HIPCHK(hipSetDevice(B->ctx->device));
  MargBatchCall c(B, W, win);
  if (int r = c.plan()) return r;
  if (int r = B->workers.parallelFor(W, [&c](const int k) { return c.prepareWindow(k); })) return r;
  if (int r = c.enqueue()) return r;
  return B->workers.parallelFor(W, [&c](const int k) { return c.finishWindow(k); });
}
int dmvio_hip_ba_batch_last_marg_ms(dmvio_hip_ba_batch* B, float* ms) {
  if (!B || !ms) return failmsg("ba_batch_last_marg_ms: null argument");
  std::lock_guard<std::mutex> lkB(B->mu);
  *ms = B->marg_ms;
  return 0;
}
int dmvio_hip_ba_batch_last_marg_work(dmvio_hip_ba_batch* B, int* launches, int* uploads, int* downloads, int* waits) {
  if (!B) return failmsg("ba_batch_last_marg_work: null batch");
  std::lock_guard<std::mutex> lkB(B->mu);
  B->marg_work.report(launches, uploads, downloads, waits);
  return 0;
}
// windows[W]: handles of the batch's context, each with its window set (set_window + set_graph), all distinct.  rmse / finalEnergy / iterations: W entries each (may be
// NULL); trace: W x 64 x 4 doubles or NULL ([E_A, E_L, E_M, accepted] per iteration, row 0 = the initial state).  Windows with different keyframe counts run as separate
// groups, one after the other.  Every window's result is what a batch of that window alone gives, bit for bit (no arithmetic crosses windows).
// Diagnostics: host clock (us since the call began) at the phase boundaries of the last dmvio_hip_ba_optimize_batch group: [0] stream hand-over done, [1] per-window tables
// prepared, [2] whole loop enqueued, [3] loop finished (first wait), [4] states written back, [5] final linearisation enqueued, [6] finished (second wait), [7] results out
int dmvio_hip_ba_batch_last_host_us(dmvio_hip_ba_batch* B, double us8[8]) {
  if (!B || !us8) return failmsg("ba_batch_last_host_us: null argument");
  std::lock_guard<std::mutex> lkB(B->mu);
  for (int k = 0; k < 8; k++) us8[k] = B->host_us[k];
  return 0;
}
int dmvio_hip_ba_optimize_batch(dmvio_hip_ba_batch* B, int W, dmvio_hip_ba* const* windows, int mnumOptIts, float* rmse, double* finalEnergy, int* iterations, double* trace) {
  if (!B || !windows || W < 1) return failmsg("ba_optimize_batch: bad argument");
  if (W > B->cap) return failmsg("ba_optimize_batch: more windows than the batch was created for");
  std::lock_guard<std::mutex> lkB(B->mu);
  HIPCHK(hipSetDevice(B->ctx->device));
  // the handles' locks, in address order (two batches sharing handles cannot deadlock)
  std::vector<dmvio_hip_ba*> order(windows, windows + W);
  std::sort(order.begin(), order.end());
  for (int i = 0; i < W; i++) {
    if (!order[i]) return failmsg("ba_optimize_batch: null window");
    if (i > 0 && order[i] == order[i - 1]) return failmsg("ba_optimize_batch: a window appears twice");
    if (order[i]->ctx != B->ctx) return failmsg("ba_optimize_batch: a window belongs to another context");
  }
  std::vector<std::unique_lock<std::recursive_mutex>> locks;
  for (dmvio_hip_ba* b : order) locks.emplace_back(b->mu);
  for (int i = 0; i < W; i++) {
    dmvio_hip_ba* b = windows[i];
    if (!b->graph_ready) return failmsg("ba_optimize_batch: set_window + set_graph first");
    if (sharded(b)) return failmsg("ba_optimize_batch: a window sharded over ranks cannot join a batch");
  }
  // groups of equal keyframe count, in the caller's order
  std::vector<char> doneW(W, 0);
  for (int i = 0; i < W; i++) {
    if (doneW[i]) continue;
    std::vector<int> idx;
    for (int j = i; j < W; j++) if (!doneW[j] && windows[j]->H.F == windows[i]->H.F) { idx.push_back(j); doneW[j] = 1; }
    const int Wn = (int)idx.size();
    std::vector<dmvio_hip_ba*> hs(Wn);
    std::vector<float> r(Wn); std::vector<double> fe(Wn), tr((size_t)BatchLayout::TRACE * Wn); std::vector<int> its(Wn);
    for (int k = 0; k < Wn; k++) hs[k] = windows[idx[k]];
    if (int rc = optimizeBatchGroup(B, Wn, hs.data(), mnumOptIts, r.data(), fe.data(), its.data(), tr.data(), nullptr)) return rc;
    for (int k = 0; k < Wn; k++) {
      if (rmse) rmse[idx[k]] = r[k];
      if (finalEnergy) finalEnergy[idx[k]] = fe[k];
      if (iterations) iterations[idx[k]] = its[k];
      if (trace) memcpy(trace + (size_t)BatchLayout::TRACE * idx[k], tr.data() + (size_t)BatchLayout::TRACE * k, sizeof(double) * BatchLayout::TRACE);
    }
  }
  return 0;
}
}  // extern "C"
