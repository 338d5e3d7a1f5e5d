// libdmvio_hip.so — C ABI of the bundle-adjustment path (include/dmvio_hip.h, "sliding-window BA" section).
#include <hip/hip_runtime.h>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <algorithm>
#include <atomic>
#include <string>

#include "../../include/dmvio_hip.h"
#include "internal.h"
#include "ba_kernels.hpp"
#include "ba_host.hpp"
#include "ba_batch_kernels.hpp"

using namespace dmv;

#include "rccl_api.h"    // the sharded iteration's collectives (loader and communicator entry points: capi_comm.hip)
#include "ba_handle.h"   // struct dmvio_hip_ba, its lock / ready checks and the transitions of the loops' caches

// The kernels whose ARGUMENTS are sized by the window (ba_kernels.hpp: BAPreDynT / ResubArgsT, the stitch workgroup of 64 F threads) take the compact instantiation up to
// BA_MAXF keyframes, the wide one up to BA_MAXF_CAP: `...` (a launch that names M_ as its template argument) once with M_ = BA_MAXF, once with BA_MAXF_CAP, the window's F picks
#define BA_BY_MAXF(F_, M_, ...) do { \
    if ((F_) <= BA_MAXF) { constexpr int M_ = BA_MAXF; __VA_ARGS__; } \
    else { constexpr int M_ = BA_MAXF_CAP; __VA_ARGS__; } \
  } while (0)

// one chunk holds the ~75 arrays of a window of 8 keyframes / 4000 points / 30k residuals; allocated (and the pinned host buffers with it) when the handle is created, so that
// no keyframe of a live system pays for hipMalloc / hipHostMalloc (seen in tests/dropin: 1.2 ms per keyframe on average over the first ten, 0.4 ms in the steady state)
static constexpr size_t BA_ARENA_CHUNK = (size_t)48 << 20;
template <class T>
static int dalloc(dmvio_hip_ba* b, T** p, size_t n) {
  if (b->arena.on) {   // inside dmvio_hip_ba_set_graph: a zeroed piece of the handle's arena
    dmvio_hip_ba::Arena& A = b->arena;
    const size_t bytes = (sizeof(T) * std::max<size_t>(n, 1) + 255) & ~(size_t)255;
    while (A.cur < A.chunks.size() && A.off + bytes > A.chunks[A.cur].second) { A.cur++; A.off = 0; }
    if (A.cur == A.chunks.size()) {
      const size_t size = std::max<size_t>(bytes, BA_ARENA_CHUNK);
      char* base = nullptr;
      HIPCHK(hipMalloc((void**)&base, size));
      HIPCHK(hipMemset(base, 0, size));
      HIPCHK(hipStreamSynchronize(nullptr));
      A.chunks.push_back(std::make_pair(base, size)); A.used.push_back(0);
      A.off = 0;
    }
    *p = reinterpret_cast<T*>(A.chunks[A.cur].first + A.off);
    A.off += bytes;
    A.used[A.cur] = std::max(A.used[A.cur], A.off);
    return 0;
  }
  HIPCHK(hipMalloc((void**)p, sizeof(T) * std::max<size_t>(n, 1)));
  HIPCHK(hipMemset(*p, 0, sizeof(T) * std::max<size_t>(n, 1)));
  // hipMemset clears on the NULL stream without blocking the host, and the handle's stream is non-blocking: without this wait an upload enqueued next could
  // land before the clear does (seen with two processes sharing a GPU)
  HIPCHK(hipStreamSynchronize(nullptr));
  b->allocs.push_back((void*)*p);
  return 0;
}
// what a new graph replaces: the arrays allocated outside the arena (exchange buffers of a sharded window); the arena's chunks and the pinned host buffers stay
static void freeDevice(dmvio_hip_ba* b) {
  for (void* p : b->allocs) hipFree(p);
  b->allocs.clear();
  b->graph_ready = false;
}
static void freeAll(dmvio_hip_ba* b) {
  freeDevice(b);
  for (auto& ch : b->arena.chunks) hipFree(ch.first);
  b->arena.chunks.clear(); b->arena.used.clear(); b->arena.cur = b->arena.off = 0;
  b->bounce.release();
  auto freeHost = [](auto*& p) { if (p) { hipHostFree(p); p = nullptr; } };
  freeHost(b->h_sys); freeHost(b->h_spart); freeHost(b->h_res); freeHost(b->h_frameTH); freeHost(b->h_idepth_backup); freeHost(b->h_pre[0]); freeHost(b->h_pre[1]);
  b->cap_spart = b->cap_idepth_backup = 0;
}

// the kernels' view of the window (calibration, frame slots, thresholds) from the host's
static void fillWindow(dmvio_hip_ba* b) {
  BAHost& H = b->H;
  BAWindow& W = b->W;
  W.F = H.F; W.w = H.w; W.h = H.h; W.N = H.N; W.R = H.R;
  W.fx = H.c_f[0]; W.fy = H.c_f[1]; W.cx = H.c_f[2]; W.cy = H.c_f[3];
  W.fxi = H.c_i[0]; W.fyi = H.c_i[1]; W.cxi = H.c_i[2]; W.cyi = H.c_i[3];
  W.wM3 = H.w - 3; W.hM3 = H.h - 3;
  W.huberTH = H.S.huberTH; W.outlierTHSum = H.S.outlierTHSumComponent; W.modeA = H.S.affineOptModeA; W.modeB = H.S.affineOptModeB;
  for (int f = 0; f < H.F; f++) { W.slot[f] = H.fr[f].slot; W.frameEnergyTH[f] = H.fr[f].frameEnergyTH; }
}
static void dynFromHost(const BAHost& H, BAPreDyn& T) {
  for (int hh = 0; hh < H.F; hh++)
    for (int t = 0; t < H.F; t++) {
      if (hh == t) continue;
      const BAPrecalc& pc = H.pre[hh + H.F * t];
      float* v = T.v[baPairIndex(hh, t, H.F)];
      for (int k = 0; k < 9; k++) v[k] = pc.KRKi[k];
      v[9] = pc.Kt[0]; v[10] = pc.Kt[1]; v[11] = pc.Kt[2]; v[12] = pc.aff0; v[13] = pc.aff1;
    }
}
// ... and the precalc table of the current state into the device table
static int uploadWindowTables(dmvio_hip_ba* b) {
  BAHost& H = b->H;
  b->evalPointUploaded();
  fillWindow(b);
  // two pinned staging copies: the previous upload may still be in flight behind a linearisation the host did not wait for (a deferred one), the one before it cannot be
  BAPrecalc* stage = b->h_pre[b->pre_toggle ^= 1];
  memcpy(stage, H.pre.data(), sizeof(BAPrecalc) * H.F * H.F);
  HIPCHK(hipMemcpyAsync(b->d_pre, stage, sizeof(BAPrecalc) * H.F * H.F, hipMemcpyHostToDevice, b->stream));
  return 0;
}
static int uploadAdjoints(dmvio_hip_ba* b) {
  b->adj_dirty = false;
  // staged in the handle's pinned area: the host tables may change (setAdjointsF of the next state) while the copy is still in flight
  HIPCHK(b->bounce.h2d(b->d_adHost, b->H.adHost.data(), sizeof(double) * b->H.adHost.size(), b->stream));
  HIPCHK(b->bounce.h2d(b->d_adTarget, b->H.adTarget.data(), sizeof(double) * b->H.adTarget.size(), b->stream));
  return 0;
}

// Completion of a chain of kernels: its last kernel stores the chain's ticket into host-coherent memory behind its results; the host spins
// on that word instead of paying a stream synchronisation (wake-up latency) per Gauss-Newton iteration.
template <class Published>
static int spinUntil(dmvio_hip_ba* b, Published published, const char* what, const char* unpublished) {
  unsigned long long spins = 0;
  while (!published()) {
    __builtin_ia32_pause();
    if ((++spins & 0xFFFFF) == 0) {
      const hipError_t q = hipStreamQuery(b->stream);
      if (q != hipSuccess && q != hipErrorNotReady) return fail(what, __FILE__, __LINE__, q);
      if (q == hipSuccess && !published()) return failmsg(unpublished);
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}
static int waitTicket(dmvio_hip_ba* b, const unsigned int ticket) {
  volatile unsigned int* flag = &b->h_res->ticket;
  return spinUntil(b, [=] { return *flag == ticket; }, "BA kernel chain", "BA kernel chain finished without publishing its ticket");
}
// the host's mirror of the newest keyframe's threshold after an accepted step: the decision pass publishes its decision first and the threshold behind it
static int resolveTh(dmvio_hip_ba* b) {
  if (!b->th_pending) return 0;
  volatile unsigned int* flag = &b->h_res->th_ticket;
  const unsigned int ticket = b->th_pending_ticket;
  if (int r = spinUntil(b, [=] { return (int)(*flag - ticket) >= 0; }, "BA decision pass", "BA decision pass finished without publishing its threshold")) return r;
  b->H.fr[b->H.F - 1].frameEnergyTH = b->h_res->th[0];
  b->th_pending = false;
  return 0;
}
static int uploadThresholds(dmvio_hip_ba* b) {
  if (int r = resolveTh(b)) return r;
  if (!b->th_dirty) return 0;
  for (int f = 0; f < BA_MAXF_CAP; f++) b->h_frameTH[f] = f < b->H.F ? b->H.fr[f].frameEnergyTH : 0.0f;
  HIPCHK(hipMemcpyAsync(b->d_frameTH, b->h_frameTH, sizeof(float) * BA_MAXF_CAP, hipMemcpyHostToDevice, b->stream));
  b->th_dirty = false;
  return 0;
}
static BADecide makeDecide(dmvio_hip_ba* b, int mode, bool update_th, bool publish) {
  BADecide D;
  memset(&D, 0, sizeof(D));
  const BAHost& H = b->H;
  D.newestE = b->d_newestE; D.n_newest = (int)b->h_newest.size(); D.newestFrame = H.F - 1;
  D.frameTH = b->d_frameTH; D.epart = b->d_epart;
  D.thN = H.S.frameEnergyTHN; D.thFacMedian = H.S.frameEnergyTHFacMedian; D.thConstWeight = H.S.frameEnergyTHConstWeight; D.overallW = H.S.overallEnergyTHWeight;
  D.thCap = b->th_cap;
  D.mode = mode; D.update_th = update_th ? 1 : 0;
  D.ctl = b->d_ctl; D.host = b->h_res;
  D.publish = publish ? 1 : 0;
  if (publish) D.ticket = ++b->ticket;
  return D;
}
#include "ba_shard_host.hpp"   // the exchange steps of a window sharded over ranks
#include "ba_loop_host.hpp"    // the host-driven Gauss-Newton loop: linearise, accumulate, the stages of one iteration, optimizeImpl
#include "ba_graph_host.hpp"   // setGraphImpl / setGraphFrom, the buffers of residuals kept linearised

extern "C" {

dmvio_hip_ba* dmvio_hip_ba_create(dmvio_hip_ctx* ctx) {
  if (!ctx) { failmsg("ba_create: null ctx"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { failmsg("ba_create: hipSetDevice failed"); return nullptr; }
  dmvio_hip_ba* b = new dmvio_hip_ba();
  b->ctx = ctx;
  if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) { failmsg("ba_create: stream creation failed"); delete b; return nullptr; }
  b->own_stream = true;
  b->H.w = ctx->w; b->H.h = ctx->h;
  {
    // everything a first keyframe would otherwise allocate: the first arena chunk, the pinned buffers the kernels store into, the staging area of the uploads
    constexpr int NMAXF = 4 + 8 * BA_MAXF_CAP;
    char* base = nullptr;
    bool ok = hipMalloc((void**)&base, BA_ARENA_CHUNK) == hipSuccess && hipMemset(base, 0, BA_ARENA_CHUNK) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
    if (ok) { b->arena.chunks.push_back(std::make_pair(base, BA_ARENA_CHUNK)); b->arena.used.push_back(0); }
    ok = ok && hipHostMalloc((void**)&b->h_sys, sizeof(double) * (2 * (NMAXF * NMAXF + NMAXF) + 1), hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&b->h_res, sizeof(BAHostRes), hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&b->h_frameTH, sizeof(float) * BA_MAXF_CAP, hipHostMallocDefault) == hipSuccess;
    for (int k = 0; k < 2 && ok; k++) ok = hipHostMalloc((void**)&b->h_pre[k], sizeof(BAPrecalc) * BA_MAXF_CAP * BA_MAXF_CAP, hipHostMallocDefault) == hipSuccess;
    b->cap_idepth_backup = 8192;
    ok = ok && hipHostMalloc((void**)&b->h_idepth_backup, sizeof(float) * b->cap_idepth_backup, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess;
    b->cap_spart = 4096;
    ok = ok && hipHostMalloc((void**)&b->h_spart, sizeof(float) * b->cap_spart, hipHostMallocDefault) == hipSuccess;
    size_t off = 0;
    ok = ok && b->bounce.reserve((size_t)4 << 20, b->stream, &off) == hipSuccess;
    b->bounce.used = 0;
    if (!ok) { failmsg("ba_create: device / pinned allocation failed"); freeAll(b); hipStreamDestroy(b->stream); delete b; return nullptr; }
  }
  // the only environment variable the library reads: a host-side timing printout of the GN loop (stderr), no effect on what is computed.  The accumulation order is
  // chosen with dmvio_hip_ba_set_accumulators alone (tests/test_capi_cpu.py greps csrc/ for other getenv calls)
  if (const char* e = getenv("DMVIO_HIP_BA_TIMING")) b->timing = atoi(e) != 0;
  return b;
}
void dmvio_hip_ba_destroy(dmvio_hip_ba* b) {
  if (!b) return;
  hipSetDevice(b->ctx->device);
  if (b->own_batch) { dmvio_hip_ba_batch_destroy(b->own_batch); b->own_batch = nullptr; }
  for (int k = 0; k < 2; k++) for (int i = 0; i < dmvio_hip_ba::COMM_EVS; i++) for (int j = 0; j < 2; j++) if (b->comm_ev[k][i][j]) hipEventDestroy(b->comm_ev[k][i][j]);
  hipStreamSynchronize(b->stream);
  if (b->timing && b->tm_graph_n > 0)
    fprintf(stderr, "[dmvio_hip_ba] set_graph over %ld calls (us/call): drain + arena memset=%.1f host lists=%.1f allocation=%.1f uploads=%.1f pinned buffers + slot table=%.1f adjoints + wait=%.1f\n", b->tm_graph_n,
            b->tm_graph[0] / b->tm_graph_n, b->tm_graph[1] / b->tm_graph_n, b->tm_graph[2] / b->tm_graph_n, b->tm_graph[3] / b->tm_graph_n, b->tm_graph[4] / b->tm_graph_n, b->tm_graph[5] / b->tm_graph_n);
  if (b->timing && b->tm.n > 0) {
    const char* names[8] = {"backup+prepare", "host solve", "step+precalc+energies+args", "launch", "wait for the decision", "accepted: sums+accumulate+stitch / rejected: relinearise", "-", "-"};
    fprintf(stderr, "[dmvio_hip_ba] GN iteration, host clock between phases (no synchronisation added) over %ld iterations (us/iter):", b->tm.n);
    for (int i = 0; i < 8; i++) fprintf(stderr, " %s=%.1f", names[i], b->tm.t[i] / b->tm.n);
    fprintf(stderr, "\n");
    if (b->d_accTicks) {   // block timeline of the LAST k_ba_accumulate launch (wall_clock64 = 100 MHz)
      std::vector<long long> tk(2 * (size_t)b->accTicksBlocks);
      hipMemcpy(tk.data(), b->d_accTicks, sizeof(long long) * tk.size(), hipMemcpyDeviceToHost);
      long long t0 = tk[0];
      for (int i = 0; i < b->accTicksBlocks; i++) t0 = std::min(t0, tk[2 * i]);
      const int F2 = b->H.F * b->H.F, lim[3] = {b->nsC, b->nsC + F2 * b->nsTop, b->accTicksBlocks};
      const char* cls[3] = {"calib", "top+E", "accD x4"};
      int i0 = 0;
      for (int c = 0; c < 3; c++) {
        double dmax = 0, dsum = 0, smax = 0, emax = 0; int argmax = -1;
        for (int i = i0; i < lim[c]; i++) {
          const double d = (tk[2 * i + 1] - tk[2 * i]) * 0.01, st = (tk[2 * i] - t0) * 0.01, en = (tk[2 * i + 1] - t0) * 0.01;
          dsum += d; if (d > dmax) { dmax = d; argmax = i - i0; } smax = std::max(smax, st); emax = std::max(emax, en);
        }
        fprintf(stderr, "[dmvio_hip_ba]   k_ba_accumulate %s blocks=%d: duration mean %.1f max %.1f us (block %d), latest start %.1f, latest end %.1f us\n", cls[c],
                lim[c] - i0, dsum / std::max(1, lim[c] - i0), dmax, argmax, smax, emax);
        i0 = lim[c];
      }
    }
  }
  if (b->d_accTicks) hipFree(b->d_accTicks);
  freeAll(b);
  if (b->own_stream && b->stream) hipStreamDestroy(b->stream);
  delete b;
}

// Accumulation order (takes effect with the next dmvio_hip_ba_set_graph): k partial accumulators per bucket, 1 <= k <= 8.
int dmvio_hip_ba_set_accumulators(dmvio_hip_ba* b, int k) {
  if (!b || k < 1 || k > 8) return failmsg("ba_set_accumulators: 1 <= k <= 8");
  BA_LOCK(b);
  b->nsTop = k; b->nsD = std::min(k, 4); b->nsC = k == 1 ? 1 : 4 * k;
  b->graph_ready = false;
  return 0;
}
// The 74-float RawResidualJacobian per residual (dmvio_hip_ba_get_jacobians) is written by the linearisation only while this is on.
int dmvio_hip_ba_keep_jacobians(dmvio_hip_ba* b, int on) {
  if (!b) return failmsg("null ba");
  BA_LOCK(b);
  b->keep_fullJ = on != 0;
  return 0;
}

// ---- communicator of a window whose points are sharded over ranks (include/dmvio_hip.h)
static int setComm(dmvio_hip_ba* b, ncclComm_t comm, const dmvio_hip_comm_callbacks* cb, int rank, int world) {
  if (!b) return failmsg("null ba");
  BA_LOCK(b);
  if (world == 0 || (!comm && !cb)) { b->world = 0; b->rank = 0; b->nccl = nullptr; b->comm_cb = dmvio_hip_comm_callbacks{}; b->stateChanged(); return 0; }
  if (world < 1 || rank < 0 || rank >= world) return failmsg("ba_set_comm: 0 <= rank < world");
  if (b->n_lin > 0) return failmsg("ba_set_comm: the graph already carries residuals kept linearised — set the communicator first, dmvio_hip_ba_fix_linearization is collective on a sharded window");
  if (cb && (!cb->allreduce_sum_f64 || !cb->allgather)) return failmsg("ba_set_comm_callbacks: both callbacks are required");
  if (comm) {
    RCCL_READY();
    int n = 0, r = -1;
    NCCLCHK(rccl().commCount(comm, &n));
    NCCLCHK(rccl().commUserRank(comm, &r));
    if (n != world || r != rank) return failmsg("ba_set_comm: rank / world do not match the communicator");
  }
  b->rank = rank; b->world = world; b->nccl = comm;
  b->comm_cb = cb ? *cb : dmvio_hip_comm_callbacks{};
  b->xchg_width = 0;            // agreed on at the next linearisation
  b->stateChanged();
  return 0;
}
int dmvio_hip_ba_set_comm(dmvio_hip_ba* b, void* nccl_comm, int rank, int world) { return setComm(b, (ncclComm_t)nccl_comm, nullptr, rank, world); }
// Measurement of the sharded iteration's two collectives (RCCL transport): on = 1 starts collecting HIP events around them on the BA stream (and clears the counters); the
// query waits for the stream and returns mean microseconds of [all-reduce of the packed system, all-gather of the decision records] over the first 64 of each since then,
// and how many of each were issued in total.  What a multi-GPU scaling line needs to explain itself (a window sharded over N GPUs pays both per iteration).
int dmvio_hip_ba_comm_timing(dmvio_hip_ba* b, int on) {
  if (!b) return failmsg("ba: null handle");
  BA_LOCK(b);
  b->comm_timing = on != 0; b->comm_n[0] = b->comm_n[1] = 0; b->comm_total[0] = b->comm_total[1] = 0;
  return 0;
}
int dmvio_hip_ba_comm_times(dmvio_hip_ba* b, double mean_us2[2], long issued2[2]) {
  if (!b || !mean_us2 || !issued2) return failmsg("ba_comm_times: null argument");
  BA_LOCK(b);
  HIPCHK(hipSetDevice(b->ctx->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  for (int k = 0; k < 2; k++) {
    double sum = 0;
    for (int i = 0; i < b->comm_n[k]; i++) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, b->comm_ev[k][i][0], b->comm_ev[k][i][1])); sum += 1e3 * ms; }
    mean_us2[k] = b->comm_n[k] ? sum / b->comm_n[k] : 0.0;
    issued2[k] = b->comm_total[k];
  }
  return 0;
}
int dmvio_hip_ba_partition_points(const int* host, int N, int world, double max_imbalance, int* owner_out) {
  if (N < 0 || world < 1 || (N > 0 && (!host || !owner_out))) return failmsg("dmvio_hip_ba_partition_points: bad argument");
  if (max_imbalance <= 0) max_imbalance = 1.25;
  int nkf = 0;
  for (int i = 0; i < N; i++) {
    if (host[i] < 0) return failmsg("dmvio_hip_ba_partition_points: negative host keyframe index");
    nkf = std::max(nkf, host[i] + 1);
  }
  if (world == 1) { for (int i = 0; i < N; i++) owner_out[i] = 0; return 0; }
  std::vector<long long> counts(nkf, 0), load(world, 0);
  for (int i = 0; i < N; i++) counts[host[i]]++;
  std::vector<int> order(nkf), owner(nkf, 0);
  for (int k = 0; k < nkf; k++) order[k] = k;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return counts[a] > counts[b]; });   // largest keyframe first, ties in index order
  for (int kf : order) {
    int r = 0;
    for (int q = 1; q < world; q++) if (load[q] < load[r]) r = q;                                       // the lightest rank, the lowest one among equals
    owner[kf] = r; load[r] += counts[kf];
  }
  const long long heaviest = *std::max_element(load.begin(), load.end());
  if ((double)heaviest > max_imbalance * std::max((double)N / world, 1.0)) {
    for (int r = 0; r < world; r++) {
      const long long lo = ((long long)N * r) / world, hi = ((long long)N * (r + 1)) / world;
      for (long long i = lo; i < hi; i++) owner_out[i] = r;
    }
    return 1;
  }
  for (int i = 0; i < N; i++) owner_out[i] = owner[host[i]];
  return 0;
}
int dmvio_hip_ba_set_comm_callbacks(dmvio_hip_ba* b, const dmvio_hip_comm_callbacks* cb, int rank, int world) { return setComm(b, nullptr, cb, rank, world); }

// The stream the mapping side enqueues on (default: a stream owned by the handle).  NULL restores an own stream.
int dmvio_hip_ba_set_stream(dmvio_hip_ba* b, void* stream) {
  if (!b) return failmsg("null ba");
  BA_LOCK(b);
  HIPCHK(hipSetDevice(b->ctx->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (b->own_stream) { HIPCHK(hipStreamDestroy(b->stream)); b->own_stream = false; }
  if (stream) b->stream = (hipStream_t)stream;
  else { HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking)); b->own_stream = true; }
  return 0;
}

int dmvio_hip_ba_max_frames(void) { return BA_MAXF_CAP; }
int dmvio_hip_ba_set_window(dmvio_hip_ba* b, int F, const int* slots, const double* pose7_w2c, const double* aff_ab, const float* exposures,
                            const int* frameIDs, const double fxfycxcy[4]) {
  if (!b || !slots || !pose7_w2c || !fxfycxcy) return failmsg("ba_set_window: null argument");
  BA_LOCK(b);
  b->stateChanged();
  if (F < 1 || F > BA_MAXF_CAP) return failmsg("ba_set_window: 1 <= F <= " + std::to_string(BA_MAXF_CAP) + " keyframes (dmvio_hip_ba_max_frames)");
  // a threshold still on its way from the previous window's last accepted step (th_ticket follows the decision) belongs to THAT window: it must neither be waited for
  // after the host-coherent record is cleared (set_graph) nor land in the new window's newest keyframe
  b->th_pending = false;
  BAHost& H = b->H;
  H.F = F;
  H.calibInitScaled(fxfycxcy);
  for (int f = 0; f < F; f++) {
    if (slots[f] < 0 || slots[f] >= b->ctx->n_slots) return failmsg("ba_set_window: frame slot out of range");
    if (int r = dmv_ensure_row_major(b->ctx, slots[f])) return r;   // the linearisation taps row-major level-0 planes (a slot the batched raw build left in tiles is converted once)
    BAFrameHost& fr = H.fr[f];
    fr = BAFrameHost();
    fr.slot = slots[f];
    fr.ab_exposure = exposures ? exposures[f] : 1.0f;
    fr.frameID = frameIDs ? frameIDs[f] : f;
    fr.evalPT = poseFrom7(pose7_w2c + 7 * f);
    const double a = aff_ab ? aff_ab[2 * f] : 0.0, bb = aff_ab ? aff_ab[2 * f + 1] : 0.0;
    double st[10] = {0, 0, 0, 0, 0, 0, (1.0f / 10.0f) * a, (1.0f / 1000.0f) * bb, 0, 0};   // setEvalPT_scaled (HessianBlocks.h:220-227)
    for (int i = 0; i < 10; i++) { fr.step[i] = 0; fr.state_backup[i] = 0; }
    BAHost::frameSetState(fr, st);
    BAHost::frameSetStateZero(fr, fr.state);
  }
  const int n = H.n();
  H.HM.assign((size_t)n * n, 0.0); H.bM.assign(n, 0.0);
  for (int f = 0; f < F; f++) H.frameTakeData(H.fr[f]);
  H.setAdjointsF();
  H.setPrecalcValues();
  b->graph_ready = false;
  b->th_dirty = true;
  return 0;
}

int dmvio_hip_ba_set_marg_prior(dmvio_hip_ba* b, const double* HM, const double* bM) {
  if (!b || !HM || !bM) return failmsg("ba_set_marg_prior: null argument");
  BA_LOCK(b);
  b->stateChanged();
  const int n = b->H.n();
  b->H.HM.assign(HM, HM + (size_t)n * n); b->H.bM.assign(bM, bM + n);
  return 0;
}

// FullSystem::flagPointsForRemoval's relinearisation (FullSystem.cpp:829-859) + EnergyFunctional::marginalizePointsF (EnergyFunctional.cpp:678-742)
int dmvio_hip_ba_marginalize_points(dmvio_hip_ba* b, const unsigned char* candidates, unsigned char* decision, double* Hadd, double* badd, int* resInM, int update_prior) {
  if (!b || !b->graph_ready) return failmsg("ba_marginalize_points: window / graph not set");
  BA_LOCK(b);
  b->stateChanged();
  if (!candidates || !decision) return failmsg("ba_marginalize_points: null argument");
  dmvio_hip_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->device));
  BAHost& H = b->H;
  const int N = H.N, R = H.R, n = H.n();
  hipStream_t s = b->stream;
  const float setting_minIdepthH_marg = BA_MARG_MIN_IDEPTH_H, setting_idepthFixPriorMargFac = BA_MARG_IDEPTH_FIX_PRIOR_FAC;
  const double setting_margWeightFac = BA_MARG_WEIGHT_FAC;
  // deltas at the current state (EnergyFunctional::setDeltaF, EnergyFunctional.cpp:175-198)
  std::vector<float> adHT;
  H.adHTdeltaF(adHT);
  HIPCHK(b->bounce.h2d(b->d_cand, candidates, N, s));
  HIPCHK(b->bounce.h2d(b->d_adHTdelta, adHT.data(), sizeof(float) * adHT.size(), s));
  // (adHT is staged in the pinned bounce: no wait)
  if (int r = uploadWindowTables(b)) return r;
  if (int r = uploadThresholds(b)) return r;
  {
    const bool fullJ_applied = b->fullJ_applied;
    const BADecide D = makeDecide(b, -1, false, false);   // masked relinearisation: no energy / threshold / accept pass
    LinearizeArgs A = linearizeArgs(b, D);
    A.fullJ = b->d_fullJ; A.mask = b->d_cand;
    launchLinearize(b, A);
    b->fullJ_applied = fullJ_applied;   // the candidates' rows are rewritten and applied right below, the others untouched
  }
  hipLaunchKernelGGL(k_ba_apply, dim3((R + 255) / 256), dim3(256), 0, s, R, b->Rs, (const unsigned char*)b->d_cand, 0);
  if (b->n_lin > 0) {   // FullSystem.cpp:840-843: a candidate point's residuals are relinearised with isLinearized = false
    for (int ri = 0; ri < R; ri++) if (candidates[b->h_point[ri]] && b->h_lin[ri]) { b->h_lin[ri] = 0; b->n_lin--; }
    HIPCHK(b->bounce.h2d(b->d_lin, b->h_lin.data(), R, s));
    if (!sharded(b)) b->n_lin_global = b->n_lin;
    if (b->n_lin == 0 && !sharded(b)) { b->Rs.lin = nullptr; b->P.lHdd = b->P.lbd = b->P.lHcd = nullptr; b->P.HcdAF = nullptr; b->H.HLraw.clear(); b->H.bLraw.clear(); }
  }
  hipLaunchKernelGGL(k_ba_marg_decide, dim3((N + 255) / 256), dim3(256), 0, s, N, b->d_cand, b->P.idepth_hessian, setting_minIdepthH_marg, b->d_decision);
  const float4 cd = make_float4(H.cDeltaF[0], H.cDeltaF[1], H.cDeltaF[2], H.cDeltaF[3]);
  hipLaunchKernelGGL(k_ba_fix_linearization, dim3((R + 255) / 256), dim3(256), 0, s, b->W, b->P, b->Rs, b->d_fullJ, b->d_decision, b->d_adHTdelta, cd, b->d_margRec,
                     b->d_margActive, (float*)nullptr);
  hipLaunchKernelGGL(k_ba_marg_point_sums, dim3(b->n_pt_blocks), dim3(256), 0, s, b->W, b->P, b->Rs, b->d_margRec, b->d_margActive, b->d_decision,
                     setting_idepthFixPriorMargFac, b->d_mHdiF, b->d_mbdSumF, b->d_mHcd);
  HIPCHK(hipGetLastError());
  BARes RsV = b->Rs; RsV.rec[0] = RsV.rec[1] = b->d_margRec; RsV.active = b->d_margActive;
  BAPoints PV = b->P; PV.HdiF = b->d_mHdiF; PV.bdSumF = b->d_mbdSumF; PV.Hcd = b->d_mHcd;
  const int resInA_keep = H.resInA;
  if (int r = accumulateViews(b, RsV, PV)) return r;
  const int nres = H.resInA;
  H.resInA = resInA_keep;
  HIPCHK(b->bounce.d2h(decision, b->d_decision, N, s));
  HIPCHK(b->bounce.finish(s));
  const double* M = b->h_sys; const double* Mb = M + (size_t)n * n; const double* Msc = Mb + n; const double* Mbsc = Msc + (size_t)n * n;
  if (H.HM.size() != (size_t)n * n) { H.HM.assign((size_t)n * n, 0.0); H.bM.assign(n, 0.0); }
  for (size_t k = 0; k < (size_t)n * n; k++) { const double v = setting_margWeightFac * (M[k] - Msc[k]); if (Hadd) Hadd[k] = v; if (update_prior) H.HM[k] += v; }
  for (int k = 0; k < n; k++) { const double v = setting_margWeightFac * (Mb[k] - Mbsc[k]); if (badd) badd[k] = v; if (update_prior) H.bM[k] += v; }
  if (resInM) *resInM = nres;
  return 0;
}

// synchronous on return, like every entry point that takes caller arrays; dmvio_hip_ba_set_graph_from is the stream-ordered form
int dmvio_hip_ba_set_graph(dmvio_hip_ba* b, int N, const int* host, const float* u, const float* v, const float* idepth, const float* color8,
                           const float* weights8, const unsigned char* hasDepthPrior, int R, const int* res_point, const int* res_target) {
  return setGraphImpl(b, N, host, u, v, idepth, color8, weights8, hasDepthPrior, R, res_point, res_target, true);
}

int dmvio_hip_ba_set_graph_from(dmvio_hip_ba* b, dmvio_hip_graph* g) {
  if (!b || !g) return failmsg("ba_set_graph_from: null argument");
  BA_LOCK(b);
  return setGraphFrom(b, g);
}

int dmvio_hip_ba_set_residual_flags(dmvio_hip_ba* b, int R, const unsigned char* isLinearized) {
  if (!b || !isLinearized) return failmsg("ba_set_residual_flags: null argument");
  BA_LOCK(b);
  if (!b->graph_ready) return failmsg("ba: set_window + set_graph first");
  if (R != b->H.R) return failmsg("ba_set_residual_flags: R differs from the graph's residual count");
  for (int ri = 0; ri < R; ri++)
    if (isLinearized[ri]) {
      b->graph_ready = false;   // refused as a whole: nothing may run on a graph whose linearised energy term (accumulateLF_MT) would be missing
      return failmsg("ba_set_residual_flags: residual " + std::to_string(ri) + " arrives linearised (EFResidual::isLinearized): its frozen Jacobian and res_toZeroF, which "
                     "accumulateLF_MT / addPoint<1> (EnergyFunctional.cpp:223-233, AccumulatedTopHessian.cpp:84-98) need, do not come with a bare flag — hand them over with "
                     "dmvio_hip_ba_set_linearized_residuals (or dmvio_hip_graph_set_residual_linearized + dmvio_hip_ba_set_graph_from); the graph is refused");
    }
  return 0;
}

// EFResidual::fixLinearizationF (EnergyFunctionalStructs.cpp:85-113) for the active residuals with res_mask != 0, at the current state, on the resident graph: from then on
// they stay out of activeResiduals (FullSystemOptimize.cpp:436-446) and enter every system through accumulateLF_MT / addPoint<1> and the energy through calcLEnergyPt, until
// the next dmvio_hip_ba_set_graph (or until their point is marginalised).  Needs the Jacobians of the applied linearisation: dmvio_hip_ba_keep_jacobians(ba, 1) before the
// dmvio_hip_ba_optimize / dmvio_hip_ba_linearize(fix) that precedes this call.  n_linearized: residuals of the graph that are linearised after the call.
int dmvio_hip_ba_fix_linearization(dmvio_hip_ba* b, int R, const unsigned char* res_mask, int* n_linearized) {
  if (!b || !res_mask) return failmsg("ba_fix_linearization: null argument");
  BA_LOCK(b);
  BA_READY_LOCKED(b);
  BAHost& H = b->H;
  if (R != H.R) return failmsg("ba_fix_linearization: R differs from the graph's residual count");
  if (!b->keep_fullJ || !b->fullJ_applied)
    return failmsg("ba_fix_linearization: the Jacobians of the applied linearisation are not resident — call dmvio_hip_ba_keep_jacobians(ba, 1) before the optimize / "
                   "linearize(fix) + apply that precedes this call");
  hipStream_t s = b->stream;
  if (int r = linAlloc(b)) return r;
  H.setPrecalcValues();
  std::vector<float> adHT;
  H.adHTdeltaF(adHT);
  HIPCHK(b->bounce.h2d(b->d_linMask, res_mask, R, s));
  HIPCHK(b->bounce.h2d(b->d_adHTdelta, adHT.data(), sizeof(float) * adHT.size(), s));
  const float4 cd = make_float4(H.cDeltaF[0], H.cDeltaF[1], H.cDeltaF[2], H.cDeltaF[3]);
  hipLaunchKernelGGL(k_ba_lin_fix, dim3((R + 255) / 256), dim3(256), 0, s, b->W, b->P, b->Rs, (const float*)b->d_fullJ, (const unsigned char*)b->d_linMask, (const float*)b->d_adHTdelta, cd,
                     b->d_lin, b->d_rtz, b->d_linRec);
  HIPCHK(hipGetLastError());
  return linFinish(b, n_linearized);
}
// EFResidual::isLinearized / J / res_toZeroF of residuals that were linearised ELSEWHERE (a graph handed over with dmvio_hip_ba_set_graph whose residuals carry the flag:
// EnergyFunctionalStructs.h:63-87), for the flagged residuals: rows of J74 (R x 74, the RawResidualJacobian in dmvio_hip_ba_get_full_jacobians' layout) and res_toZeroF
// (R x 8); the rows of the others are not read.  They become what dmvio_hip_ba_fix_linearization leaves behind.
int dmvio_hip_ba_set_linearized_residuals(dmvio_hip_ba* b, int R, const unsigned char* isLinearized, const float* J74, const float* res_toZeroF, int* n_linearized) {
  if (!b || !isLinearized || !J74 || !res_toZeroF) return failmsg("ba_set_linearized_residuals: null argument");
  BA_LOCK(b);
  BA_READY_LOCKED(b);
  if (R != b->H.R) return failmsg("ba_set_linearized_residuals: R differs from the graph's residual count");
  return linImport(b, isLinearized, J74, res_toZeroF, n_linearized);
}
// ... and back: EFResidual::isLinearized / J / res_toZeroF of the graph's residuals as they stand (linearised here or handed over) — what an adapter writes back into the
// reference's objects, or hands to the next window's dmvio_hip_graph_set_residual_linearized.  Rows of residuals that are not linearised are zeroed.  Any output may be NULL.
int dmvio_hip_ba_get_linearized_residuals(dmvio_hip_ba* b, int R, unsigned char* isLinearized, float* J74, float* res_toZeroF) {
  if (!b) return failmsg("ba: null handle");
  BA_LOCK(b);
  if (!b->graph_ready) return failmsg("ba: set_window + set_graph first");
  if (R != b->H.R) return failmsg("ba_get_linearized_residuals: R differs from the graph's residual count");
  const bool have = b->d_lin != nullptr && (int)b->h_lin.size() == R && b->h_linJ.size() == (size_t)R * FJ_FLOATS;
  for (int ri = 0; ri < R; ri++) {
    const bool l = have && b->h_lin[ri];
    if (isLinearized) isLinearized[ri] = l ? 1 : 0;
    if (J74) { if (l) memcpy(J74 + (size_t)ri * FJ_FLOATS, &b->h_linJ[(size_t)ri * FJ_FLOATS], sizeof(float) * FJ_FLOATS); else memset(J74 + (size_t)ri * FJ_FLOATS, 0, sizeof(float) * FJ_FLOATS); }
    if (res_toZeroF) { if (l) memcpy(res_toZeroF + (size_t)ri * 8, &b->h_rtz[(size_t)ri * 8], sizeof(float) * 8); else memset(res_toZeroF + (size_t)ri * 8, 0, sizeof(float) * 8); }
  }
  return 0;
}
// accumulateLF_MT's system as the reference returns it (stitched linearised residuals + priors, EnergyFunctional.cpp:223-233) for the state of the LAST accumulation
// (dmvio_hip_ba_accumulate / _solve / _optimize); without residuals kept linearised it holds the priors only
int dmvio_hip_ba_get_lf_system(dmvio_hip_ba* b, double* HL, double* bL) {
  if (!b) return failmsg("ba: null handle");
  BA_LOCK(b);
  if (!b->graph_ready) return failmsg("ba: set_window + set_graph first");
  const BAHost& H = b->H;
  const int n = H.n();
  double HLd[4 + 8 * BA_MAXF_CAP], bLv[4 + 8 * BA_MAXF_CAP];
  const bool haveL = H.lfTop(HLd, bLv);
  if (HL) for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) HL[(size_t)i * n + j] = (haveL ? H.HLraw[(size_t)i * n + j] : 0.0) + (i == j ? HLd[i] : 0.0);
  if (bL) memcpy(bL, bLv, sizeof(double) * n);
  return 0;
}

// activeResiduals of FullSystem::optimize: every residual is (re)activated: resetOOB (FullSystemOptimize.cpp:431-448)
int dmvio_hip_ba_activate_all(dmvio_hip_ba* b) {
  BA_READY(b);
  hipStream_t s = b->stream;
  // every residual still in the graph; those an earlier fix-linearisation deleted (FullSystemOptimize.cpp:195-212) stay out
  hipLaunchKernelGGL(k_ba_reset_oob, dim3((b->H.R + 255) / 256), dim3(256), 0, s, b->H.R, b->Rs);
  HIPCHK(hipGetLastError());
  return 0;
}
int dmvio_hip_ba_linearize(dmvio_hip_ba* b, int fix, double* energy) {
  BA_READY(b);
  double e = 0;
  if (int r = linearizeAll(b, fix != 0, TH_UPDATE, &e)) return r;
  if (energy) *energy = e;
  return 0;
}
int dmvio_hip_ba_apply(dmvio_hip_ba* b) {
  BA_READY(b);
  return applyRes(b);
}
int dmvio_hip_ba_get_res_state(dmvio_hip_ba* b, unsigned char* newState, float* newEnergy, float* newEnergyWO, unsigned char* active, float* center3) {
  BA_READY(b);
  hipStream_t s = b->stream;
  const int R = b->H.R;
  if (newState) HIPCHK(b->bounce.d2h(newState, b->Rs.newState, R, s));
  if (newEnergy) HIPCHK(b->bounce.d2h(newEnergy, b->Rs.newEnergy, sizeof(float) * R, s));
  if (active) HIPCHK(b->bounce.d2h(active, b->Rs.active, R, s));
  if (center3) HIPCHK(b->bounce.d2h(center3, b->Rs.center, sizeof(float) * 3 * R, s));
  if (newEnergyWO) HIPCHK(b->bounce.d2h(newEnergyWO, b->d_newEnergyWO, sizeof(float) * R, s));
  HIPCHK(b->bounce.finish(s));
  return 0;
}
// RawResidualJacobian of the LAST linearisation (74 floats per residual, RawResidualJacobian.h:32-61 order) — parity/debug
int dmvio_hip_ba_get_jacobians(dmvio_hip_ba* b, float* J74) {
  BA_READY(b);
  if (!b->keep_fullJ) return failmsg("ba_get_jacobians: call dmvio_hip_ba_keep_jacobians(ba, 1) before the linearisation");
  HIPCHK(b->bounce.d2h(J74, b->d_fullJ, sizeof(float) * FJ_FLOATS * b->H.R, b->stream));
  HIPCHK(b->bounce.finish(b->stream));
  return 0;
}
int dmvio_hip_ba_get_frame_energy_th(dmvio_hip_ba* b, float* th) {
  if (!b || !th) return failmsg("null argument");
  BA_LOCK(b);
  if (int r = resolveTh(b)) return r;
  for (int f = 0; f < b->H.F; f++) th[f] = b->H.fr[f].frameEnergyTH;
  return 0;
}
int dmvio_hip_ba_accumulate(dmvio_hip_ba* b, double* HA, double* bA, double* Hsc, double* bsc, int* resInA) {
  BA_READY(b);
  if (int r = accumulate(b)) return r;
  const int n = b->H.n();
  const double* p = b->h_sys;
  if (HA) memcpy(HA, p, sizeof(double) * n * n);
  if (bA) memcpy(bA, p + n * n, sizeof(double) * n);
  if (Hsc) memcpy(Hsc, p + n * n + n, sizeof(double) * n * n);
  if (bsc) memcpy(bsc, p + 2 * n * n + n, sizeof(double) * n);
  if (resInA) *resInA = b->H.resInA;
  return 0;
}
int dmvio_hip_ba_get_point_acc(dmvio_hip_ba* b, float* Hdd, float* bd, float* Hcd4, float* HdiF, float* bdSumF) {
  BA_READY(b);
  hipStream_t s = b->stream;
  const int N = b->H.N;
  if (Hdd) HIPCHK(b->bounce.d2h(Hdd, b->P.Hdd, sizeof(float) * N, s));
  if (bd) HIPCHK(b->bounce.d2h(bd, b->P.bd, sizeof(float) * N, s));
  if (Hcd4) HIPCHK(b->bounce.d2h(Hcd4, linAny(b) ? b->P.HcdAF : b->P.Hcd, sizeof(float) * 4 * N, s));   // Hcd_accAF
  if (HdiF) HIPCHK(b->bounce.d2h(HdiF, b->P.HdiF, sizeof(float) * N, s));
  if (bdSumF) HIPCHK(b->bounce.d2h(bdSumF, b->P.bdSumF, sizeof(float) * N, s));
  HIPCHK(b->bounce.finish(s));
  return 0;
}
// EnergyFunctional::solveSystemF: accumulate on the device, solve on the host (the hand-off point of
// BAGTSAMIntegration::computeBAUpdate in VIO mode, EnergyFunctional.cpp:958-969), back-substitute on the device.
int dmvio_hip_ba_solve(dmvio_hip_ba* b, int iteration, double lambda, double* x_out) {
  BA_READY(b);
  if (int r = accumulate(b)) return r;
  const int n = b->H.n();
  const double* p = b->h_sys;
  std::vector<double> x;
  b->H.solveSystem(iteration, lambda, p, p + n * n, p + n * n + n, p + 2 * n * n + n, x);
  if (x_out) memcpy(x_out, x.data(), sizeof(double) * n);
  return resubstitute(b, x);
}
int dmvio_hip_ba_resubstitute(dmvio_hip_ba* b, const double* x) {
  BA_READY(b);
  std::vector<double> xv(x, x + b->H.n());
  return resubstitute(b, xv);
}
int dmvio_hip_ba_get_point_hessian(dmvio_hip_ba* b, float* idepth_hessian) {
  if (!b || !b->graph_ready || !idepth_hessian) return failmsg("ba_get_point_hessian: bad argument");   // a pure read: the loop state (sys_ready) is left alone
  BA_LOCK(b);
  HIPCHK(hipSetDevice(b->ctx->device));
  HIPCHK(b->bounce.d2h(idepth_hessian, b->P.idepth_hessian, sizeof(float) * b->H.N, b->stream));
  HIPCHK(b->bounce.finish(b->stream));
  return 0;
}
int dmvio_hip_ba_get_points(dmvio_hip_ba* b, float* idepth, float* step) {
  BA_READY(b);
  hipStream_t s = b->stream;
  if (idepth) HIPCHK(b->bounce.d2h(idepth, b->P.idepth, sizeof(float) * b->H.N, s));
  if (step) HIPCHK(b->bounce.d2h(step, b->P.step, sizeof(float) * b->H.N, s));
  HIPCHK(b->bounce.finish(s));
  return 0;
}
int dmvio_hip_ba_get_frame(dmvio_hip_ba* b, int f, double pose7_w2c[7], double aff[2], double state10[10]) {
  if (!b || f < 0 || f >= b->H.F) return failmsg("ba_get_frame: bad argument");
  BA_LOCK(b);
  const BAFrameHost& fr = b->H.fr[f];
  if (pose7_w2c) poseTo7(fr.w2c, pose7_w2c);
  if (aff) { aff[0] = fr.state_scaled[6]; aff[1] = fr.state_scaled[7]; }
  if (state10) memcpy(state10, fr.state, sizeof(double) * 10);
  return 0;
}
// EnergyFunctional::marginalizeFrame (EnergyFunctional.cpp:520-660), visual-only branch: the marginalisation prior of the window
// without keyframe `frame` ((n-8) x (n-8), n-8); also returns the current prior when HM_cur / bM_cur are given.
int dmvio_hip_ba_marginalize_frame(dmvio_hip_ba* b, int frame, double* HM_new, double* bM_new) {
  if (!b || !HM_new || !bM_new || frame < 0 || frame >= b->H.F) return failmsg("ba_marginalize_frame: bad argument");
  BA_LOCK(b);
  std::vector<double> Hn, bn;
  b->H.marginalizeFrame(frame, Hn, bn);
  memcpy(HM_new, Hn.data(), sizeof(double) * Hn.size());
  memcpy(bM_new, bn.data(), sizeof(double) * bn.size());
  return 0;
}
int dmvio_hip_ba_get_marg_prior(dmvio_hip_ba* b, double* HM, double* bM) {
  if (!b || !HM || !bM) return failmsg("ba_get_marg_prior: null argument");
  BA_LOCK(b);
  const int n = b->H.n();
  if (b->H.HM.size() != (size_t)n * n) { memset(HM, 0, sizeof(double) * n * n); memset(bM, 0, sizeof(double) * n); return 0; }
  memcpy(HM, b->H.HM.data(), sizeof(double) * n * n); memcpy(bM, b->H.bM.data(), sizeof(double) * n);
  return 0;
}
// FrameHessian::setState (HessianBlocks.h:179-199) for one keyframe of the window, followed by FullSystem::setPrecalcValues
int dmvio_hip_ba_set_frame_state(dmvio_hip_ba* b, int f, const double state10[10]) {
  if (!b || !state10 || f < 0 || f >= b->H.F) return failmsg("ba_set_frame_state: bad argument");
  BA_LOCK(b);
  b->stateChanged();
  BAHost::frameSetState(b->H.fr[f], state10);
  b->H.setPrecalcValues();
  return 0;
}
// Windows taken over from a running system (rather than built fresh): FrameHessian::state_zero (HessianBlocks.cpp:74-107), frameEnergyTH
// of every keyframe and CalibHessian::value_zero (unscaled units) where they differ from what dmvio_hip_ba_set_window starts with.
int dmvio_hip_ba_set_frame_zero(dmvio_hip_ba* b, int f, const double state_zero10[10]) {
  if (!b || !state_zero10 || f < 0 || f >= b->H.F) return failmsg("ba_set_frame_zero: bad argument");
  BA_LOCK(b);
  b->stateChanged();
  BAHost::frameSetStateZero(b->H.fr[f], state_zero10);
  b->evalPointChanged();
  b->H.frameTakeData(b->H.fr[f]);
  b->H.setPrecalcValues();
  return 0;
}
int dmvio_hip_ba_set_frame_states(dmvio_hip_ba* b, const double* state_zero10, const double* state10) {
  if (!b || b->H.F < 1) return failmsg("ba_set_frame_states: bad argument");
  BA_LOCK(b);
  b->stateChanged();
  for (int f = 0; f < b->H.F; f++) {
    if (state_zero10) { BAHost::frameSetStateZero(b->H.fr[f], state_zero10 + 10 * f); b->H.frameTakeData(b->H.fr[f]); }
    if (state10) BAHost::frameSetState(b->H.fr[f], state10 + 10 * f);
  }
  if (state_zero10) b->evalPointChanged();
  b->H.setPrecalcValues();
  return 0;
}
int dmvio_hip_ba_set_frame_energy_th(dmvio_hip_ba* b, const float* th) {
  if (!b || !th) return failmsg("ba_set_frame_energy_th: null argument");
  BA_LOCK(b);
  b->th_pending = false;
  for (int f = 0; f < b->H.F; f++) b->H.fr[f].frameEnergyTH = th[f];
  b->th_dirty = true;
  return 0;
}
// IMUIntegration::newFrameEnergyTH (src/IMU/IMUIntegration.cpp:365-373, called from FullSystem::setNewFrameEnergyTH, FullSystemOptimize.cpp:136-140, when setting_useIMU):
// IMUSettings::maxFrameEnergyThreshold caps the newest keyframe's threshold; <= 0 = no cap (the reference's default)
int dmvio_hip_ba_set_frame_energy_th_cap(dmvio_hip_ba* b, float maxFrameEnergyThreshold) {
  if (!b) return failmsg("ba_set_frame_energy_th_cap: null handle");
  BA_LOCK(b);
  b->th_cap = maxFrameEnergyThreshold;
  return 0;
}
int dmvio_hip_ba_set_calib_values(dmvio_hip_ba* b, const double value[4], const double value_zero[4]) {
  if (!b || !value || !value_zero) return failmsg("ba_set_calib_values: null argument");
  BA_LOCK(b);
  b->stateChanged();
  for (int i = 0; i < 4; i++) b->H.c_value_zero[i] = value_zero[i];
  b->H.calibSetValue(value);
  b->H.setPrecalcValues();
  return 0;
}
int dmvio_hip_ba_get_calib_values(dmvio_hip_ba* b, double value[4], double value_zero[4]) {
  if (!b) return failmsg("null ba");
  BA_LOCK(b);
  if (value) memcpy(value, b->H.c_value, sizeof(double) * 4);
  if (value_zero) memcpy(value_zero, b->H.c_value_zero, sizeof(double) * 4);
  return 0;
}
int dmvio_hip_ba_get_res_in_a(dmvio_hip_ba* b, int* resInA) {
  if (!b || !resInA) return failmsg("null argument");
  BA_LOCK(b);
  *resInA = b->H.resInA;
  return 0;
}
int dmvio_hip_ba_get_calib(dmvio_hip_ba* b, double fxfycxcy[4]) {
  if (!b) return failmsg("null ba");
  BA_LOCK(b);
  memcpy(fxfycxcy, b->H.c_value_scaled, sizeof(double) * 4);
  return 0;
}

// Measurement: mean microseconds of the five kernels of an ACCEPTED Gauss-Newton iteration's chain on the current state (ba_loop_host.hpp: profileChain)
int dmvio_hip_ba_profile_chain(dmvio_hip_ba* b, int reps, float us5[5]) {
  BA_READY(b);
  if (!us5 || reps < 1) return failmsg("ba_profile_chain: bad argument");
  if (sharded(b)) return failmsg("ba_profile_chain: single-device windows only");
  return profileChain(b, reps, us5);
}

// diagnostics: in-kernel timeline of the last decision pass, 100 MHz ticks since its workgroup started (begin, energy, keys, selected)
int dmvio_hip_ba_last_decide_ticks(dmvio_hip_ba* b, int ticks4[4]) {
  if (!b || !b->h_res || !ticks4) return failmsg("null argument");
  BA_LOCK(b);
  for (int i = 0; i < 4; i++) ticks4[i] = b->h_res->ticks[i];
  return 0;
}

int dmvio_hip_ba_gn_iteration(dmvio_hip_ba* b, int iteration, double* lambda_io, double lastE[3], int* accepted) {
  if (!b) return failmsg("ba: null handle");
  BA_LOCK(b);
  BA_CHECK_LOCKED(b);
  double lam = *lambda_io;
  const GnResult g = gnIteration(b, iteration, lam, lastE, GnOpts{});
  if (g.rc) return g.rc;
  *lambda_io = lam;
  if (accepted) *accepted = g.accepted ? 1 : 0;
  return 0;
}

// ---- building blocks of a SHARDED Gauss-Newton iteration (one keyframe's points per GPU): the caller sums the packed
// local systems / energies of all ranks (RCCL all-reduce) between these calls; every rank then solves the identical reduced system.
int dmvio_hip_ba_backup(dmvio_hip_ba* b) {
  BA_READY(b);
  b->H.backupFrames();
  return pointStep(b, 0, 0.f);
}
int dmvio_hip_ba_solve_system(dmvio_hip_ba* b, int iteration, double lambda, const double* HA, const double* bA, const double* Hsc, const double* bsc, double* x_out) {
  BA_READY(b);
  if (!HA || !bA || !Hsc || !bsc) return failmsg("ba_solve_system: null argument");
  std::vector<double> x;
  b->H.solveSystem(iteration, lambda, HA, bA, Hsc, bsc, x);
  if (x_out) memcpy(x_out, x.data(), sizeof(double) * b->H.n());
  return resubstitute(b, x);
}
int dmvio_hip_ba_step(dmvio_hip_ba* b, float stepfac, float sums6[6]) {
  BA_READY(b);
  float fs[4], sumID = 0, sumNID = 0;
  b->H.stepFrames(stepfac, fs);
  if (int r = pointStep(b, 1, stepfac, &sumID, &sumNID)) return r;
  b->H.setPrecalcValues();
  if (sums6) { for (int i = 0; i < 4; i++) sums6[i] = fs[i]; sums6[4] = sumID * b->H.N; sums6[5] = sumNID * b->H.N; }  // point sums un-normalised (local shard)
  return 0;
}
int dmvio_hip_ba_restore(dmvio_hip_ba* b) {
  BA_READY(b);
  b->H.restoreFrames();
  if (int r = pointStep(b, 2, 0.f)) return r;
  b->H.setPrecalcValues();
  return 0;
}
// linearizeAll WITHOUT the setNewFrameEnergyTH tail: returns the local energy and the state_NewEnergyWithOutlier values of the local
// residuals that target the newest keyframe (the inputs of setNewFrameEnergyTH, FullSystemOptimize.cpp:96-149) so the caller can
// gather them over all shards.
int dmvio_hip_ba_linearize_local(dmvio_hip_ba* b, int fix, double* energy, float* new_frame_energies, int* n_new_frame_energies) {
  BA_READY(b);
  double e = 0;
  if (int r = linearizeAll(b, fix != 0, TH_KEEP, &e)) return r;   // the threshold is set by the caller from the energies gathered over all shards
  if (energy) *energy = e;
  std::vector<float> wo(b->H.R);
  if (b->H.R) HIPCHK(b->bounce.d2h(wo.data(), b->d_newEnergyWO, sizeof(float) * b->H.R, b->stream));
  HIPCHK(b->bounce.finish(b->stream));
  int n = 0;
  for (int ri : b->h_newest)
    if (wo[ri] >= 0) { if (new_frame_energies) new_frame_energies[n] = wo[ri]; n++; }
  if (n_new_frame_energies) *n_new_frame_energies = n;
  return 0;
}
int dmvio_hip_ba_set_new_frame_energy_th(dmvio_hip_ba* b, float th) {
  if (!b) return failmsg("null ba");
  BA_LOCK(b);
  b->stateChanged();
  b->H.fr[b->H.F - 1].frameEnergyTH = th;
  b->th_dirty = true;
  return 0;
}
int dmvio_hip_ba_energy_terms(dmvio_hip_ba* b, double* EL, double* EM) {
  if (!b) return failmsg("null ba");
  BA_LOCK(b);
  if (EL) { if (int r = calcLEnergyR(b, EL)) return r; }
  if (EM) *EM = b->H.calcMEnergy();
  return 0;
}

int dmvio_hip_ba_optimize(dmvio_hip_ba* b, int mnumOptIts, float* rmse, double* finalEnergy, int* iterations, double* trace /* 64x4 or NULL */) {
  BA_READY(b);
  if (b->device_loop && !sharded(b)) {
    if (!b->own_batch) b->own_batch = dmvio_hip_ba_batch_create(b->ctx, 1);
    if (!b->own_batch) return -1;
    dmvio_hip_ba* one = b;
    return dmvio_hip_ba_optimize_batch(b->own_batch, 1, &one, mnumOptIts, rmse, finalEnergy, iterations, trace);
  }
  return optimizeImpl(b, mnumOptIts, nullptr, nullptr, rmse, finalEnergy, iterations, trace);
}
// FullSystem::optimize with the reference's DEFAULT solver branch (settings.cpp:37 setting_useGTSAMIntegration = true): the same device-resident loop, the solve and
// the GTSAM energy term handed to the caller (include/dmvio_hip.h).
int dmvio_hip_ba_optimize_vio(dmvio_hip_ba* b, int mnumOptIts, const dmvio_hip_ba_callbacks* cb, const dmvio_hip_ba_vio_options* opt, float* rmse, double* finalEnergy,
                              int* iterations, double* trace) {
  BA_READY(b);
  if (!cb || !cb->computeBAUpdate) return failmsg("ba_optimize_vio: the computeBAUpdate hook is required (dmvio_hip_ba_optimize runs the library's own solver)");
  if (sharded(b)) return failmsg("ba_optimize_vio: not available for a window sharded over ranks (every rank would have to run identical hooks)");
  return optimizeImpl(b, mnumOptIts, cb, opt, rmse, finalEnergy, iterations, trace);
}
// dmvio_hip_ba_solve_ldlt with the signature of the computeBAUpdate hook: a ready-made hook for callers that fall back to the visual-only solve (user is ignored)
int dmvio_hip_ba_hook_ldlt(void* user, int n, const double* HPassed, const double* b_in, double lambda, const double* HNoLambda, int F, const dmvio_hip_ba_frame_view* frames,
                           const double calib_value[4], double* x_out) {
  (void)user; (void)lambda; (void)HNoLambda; (void)F; (void)frames; (void)calib_value;
  return dmvio_hip_ba_solve_ldlt(n, HPassed, b_in, x_out);
}
// The library's own solver as a computeBAUpdate hook (EnergyFunctional.cpp:971-973: diagonal pre-scaling (H_ii + 10)^-1/2, pivoted LDL^T): for hooks that fall back to the
// visual-only step, and the check that the hook path reproduces dmvio_hip_ba_optimize bit for bit.  HPassed is n x n row-major; host-only.
int dmvio_hip_ba_solve_ldlt(int n, const double* HPassed, const double* b_in, double* x_out) {
  if (!HPassed || !b_in || !x_out || n < 1 || n > 4 + 8 * BA_MAXF_CAP) return failmsg("ba_solve_ldlt: bad argument");
  std::vector<double> Ht((size_t)n * n, 0.0);
  double sv[4 + 8 * BA_MAXF_CAP], bs[4 + 8 * BA_MAXF_CAP];
  for (int i = 0; i < n; i++) sv[i] = 1.0 / std::sqrt(HPassed[(size_t)i * n + i] + 10);
  for (int i = 0; i < n; i++) { for (int j = 0; j <= i; j++) Ht[(size_t)j * n + i] = sv[i] * HPassed[(size_t)i * n + j] * sv[j]; bs[i] = sv[i] * b_in[i]; }
  BAHost::ldltSolveTransposed(Ht.data(), n, bs, n);
  for (int i = 0; i < n; i++) x_out[i] = sv[i] * bs[i];
  return 0;
}

}  // extern "C"

#include "ba_batch_host.hpp"
#include "ba_graph_batch_host.hpp"   // dmvio_hip_ba_set_graph_from_batch: the hand-over of W windows per call, on the batch object above

extern "C" {
// dmvio_hip_ba_optimize of this handle through the device-resident loop (a batch of one window, created on first use): no PCIe poll per iteration.  The host-driven loop
// (default) stays the reference for the hook branch (dmvio_hip_ba_optimize_vio), which needs the host in every iteration anyway.
int dmvio_hip_ba_set_device_loop(dmvio_hip_ba* b, int on) {
  if (!b) return failmsg("ba: null handle");
  BA_LOCK(b);
  b->device_loop = on != 0;
  return 0;
}
// the last solve's x (n = 4 + 8F doubles, MINUS the step: EnergyFunctional::lastX) of the last optimize / gn_iteration / solve of this window
int dmvio_hip_ba_get_last_x(dmvio_hip_ba* b, double* x_out) {
  if (!b || !x_out) return failmsg("ba_get_last_x: null argument");
  BA_LOCK(b);
  if ((int)b->H.lastX.size() != b->H.n()) return failmsg("ba_get_last_x: no solve yet");
  memcpy(x_out, b->H.lastX.data(), sizeof(double) * b->H.n());
  return 0;
}
}  // extern "C"
// internal.h: what dmvio_hip_tracker_set_ref_from_ba borrows of this handle
void dmv_ba_lock(dmvio_hip_ba* b) { b->mu.lock(); }
void dmv_ba_unlock(dmvio_hip_ba* b) { b->mu.unlock(); }
void dmv_ba_ref_source_locked(dmvio_hip_ba* b, DmvBaRefSource* out) {
  out->ctx = b->ctx; out->stream = b->stream;
  out->graph_ready = b->graph_ready; out->sharded = b->world != 0;
  out->F = b->H.F; out->N = b->graph_ready ? b->H.N : 0; out->R = b->graph_ready ? b->H.R : 0;   // without a graph the counts are an older window's
  out->res_point = b->Rs.point; out->res_target = b->Rs.target;
  out->newState = b->Rs.newState; out->active = b->Rs.active;
  out->center = b->Rs.center; out->HdiF = b->P.HdiF;
}
