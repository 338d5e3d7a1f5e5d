// libdmvio_hip.so — C ABI implementation (include/dmvio_hip.h), the coarse tracker: the handle's life, the evaluation server, the batched LM pipeline, the host LM, the
// try loop of trackNewCoarse and the multi-window launch.  gfx950 only.  The only unit that compiles tracker_kernels.hpp, so every launch of one of its kernels is here; the
// reference template is capi_ref.hip's.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>
#include <chrono>
#include <algorithm>
#include <atomic>

#include "../../include/dmvio_hip.h"
#include "common.h"
#include "lie_dev.h"
#include "tracker_kernels.hpp"

using namespace dmv;

#include "tracker_handle.h"

extern "C" {

// ------------------------------------------------------------------ tracker
// geometry and device memory of a fresh tracker; on failure the caller destroys the partial handle
static int trackerInit(dmvio_hip_tracker* t) {
  dmvio_hip_ctx* c = t->ctx;
  t->dev.levels = c->levels;
  t->dev.huberTH = 9.0f; t->dev.coarseCutoffTH = 20.0f; t->dev.modeA = 1e12f; t->dev.modeB = 1e8f;
  t->dev.ref_exposure = 1.0f; t->dev.ref_aff_a = 0; t->dev.ref_aff_b = 0;
  RefLevels& R = t->R;
  R.levels = c->levels;
  size_t off = 0; int tiles = 0;
  for (int l = 0; l < c->levels; l++) {
    R.w[l] = c->wl[l]; R.h[l] = c->hl[l]; R.off[l] = off; R.tile_off[l] = tiles;
    off += (size_t)R.w[l] * R.h[l];
    R.blocks_x[l] = (R.w[l] + 15) / 16;
    tiles += R.blocks_x[l] * ((R.h[l] + 15) / 16);
    t->dev.g[l].w = R.w[l]; t->dev.g[l].h = R.h[l];
  }
  R.tile_off[c->levels] = tiles; R.total = off; t->n_tiles = tiles;
  R.seg_x0 = (R.w[0] + 7) / 8;
  R.order = 0;
  {
    int so = 0;
    for (int l = 0; l < c->levels; l++) { R.seg_x[l] = (R.w[l] + 7) / 8; R.seg_off[l] = so; so += R.seg_x[l] * R.h[l]; }
    R.seg_off[c->levels] = so;
  }
  t->flow_words = ((size_t)R.w[0] * R.h[0] + 63) / 64;
  HIPCHK(hipMalloc((void**)&t->d_seg, sizeof(int) * R.seg_off[c->levels]));
  HIPCHK(hipMalloc((void**)&t->d_flow_mask, sizeof(unsigned long long) * t->flow_words));
  HIPCHK(hipMemset(t->d_flow_mask, 0, sizeof(unsigned long long) * t->flow_words));
  t->dev.flow_mask = t->d_flow_mask;
  HIPCHK(hipMalloc((void**)&t->d_idp, sizeof(float) * off));
  HIPCHK(hipMalloc((void**)&t->d_wsp, sizeof(float) * off));
  HIPCHK(hipMalloc((void**)&t->d_idp2, sizeof(float) * off));
  HIPCHK(hipMalloc((void**)&t->d_wsp2, sizeof(float) * off));
  HIPCHK(hipMalloc((void**)&t->d_dense, sizeof(float) * off));
  HIPCHK(hipMalloc((void**)&t->d_tile_count, sizeof(int) * tiles));
  HIPCHK(hipMalloc((void**)&t->d_tile_base, sizeof(int) * tiles));
  HIPCHK(hipMalloc((void**)&t->d_pc_n, sizeof(int) * dmvio_hip_tracker::PC_N_INTS));   // pc_n, then the two counters of set_ref_from_ba (tracker_handle.h)
  for (int l = 0; l < c->levels; l++) HIPCHK(hipMalloc((void**)&t->d_pc[l], sizeof(float4) * R.w[l] * R.h[l]));
  HIPCHK(hipMalloc((void**)&t->d_pc_ptrs, sizeof(float4*) * DMV_MAX_LEVELS));
  HIPCHK(hipMemcpy(t->d_pc_ptrs, t->d_pc, sizeof(float4*) * DMV_MAX_LEVELS, hipMemcpyHostToDevice));
  HIPCHK(hipMalloc((void**)&t->d_partials, sizeof(float) * ACC_PAD * t->max_eval_blocks));
  // host-coherent (fine-grained) pinned memory: the fused evaluation stores its sums and then a ticket there, the host spins on the ticket
  HIPCHK(hipHostMalloc((void**)&t->h_tot, sizeof(float) * (ACC_PAD + 16), hipHostMallocCoherent | hipHostMallocMapped));
  memset(t->h_tot, 0, sizeof(float) * (ACC_PAD + 16));
  HIPCHK(hipHostMalloc((void**)&t->h_mail, sizeof(unsigned int) * EVAL_MAIL_DWORDS, hipHostMallocCoherent | hipHostMallocMapped));
  memset(t->h_mail, 0, sizeof(unsigned int) * EVAL_MAIL_DWORDS);
  HIPCHK(hipHostMalloc((void**)&t->h_rec, sizeof(float) * EVAL_RECORD_FLOATS * EVAL_SERVER_MAX_BLOCKS, hipHostMallocCoherent | hipHostMallocMapped));
  memset(t->h_rec, 0, sizeof(float) * EVAL_RECORD_FLOATS * EVAL_SERVER_MAX_BLOCKS);
  HIPCHK(hipMalloc((void**)&t->d_arrive, sizeof(unsigned int)));
  HIPCHK(hipMemset(t->d_arrive, 0, sizeof(unsigned int)));
  HIPCHK(hipMalloc((void**)&t->d_leave, sizeof(unsigned int)));
  HIPCHK(hipMemset(t->d_leave, 0xFF, sizeof(unsigned int)));
  HIPCHK(hipStreamSynchronize(nullptr));   // the clears above run on the NULL stream; the context's stream does not wait for it
  return 0;
}

dmvio_hip_tracker* dmvio_hip_tracker_create(dmvio_hip_ctx* c) {
  if (!c) { failmsg("tracker_create: null ctx"); return nullptr; }
  HIPCHKP(hipSetDevice(c->device));
  dmvio_hip_tracker* t = new dmvio_hip_tracker();
  t->ctx = c;
  if (trackerInit(t)) { dmvio_hip_tracker_destroy(t); return nullptr; }   // releases what was allocated; the error text stays
  return t;
}

void dmvio_hip_tracker_destroy(dmvio_hip_tracker* t) {
  if (!t) return;
  hipSetDevice(t->ctx->device);
  hipStreamSynchronize(t->ctx->stream);
  t->xchg = nullptr;   // the exchange owns a device buffer (RCCL transport): released now, while the context it was allocated under is still alive
  hipFree(t->d_idp); hipFree(t->d_wsp); hipFree(t->d_idp2); hipFree(t->d_wsp2); hipFree(t->d_dense);
  hipFree(t->d_tile_count); hipFree(t->d_tile_base); hipFree(t->d_pc_n); hipFree(t->d_seg); hipFree(t->d_flow_mask);
  if (t->d_pp_next) hipFree(t->d_pp_next);
  if (t->d_ba_crowded) hipFree(t->d_ba_crowded);
  if (t->ev_ba_ready) hipEventDestroy(t->ev_ba_ready);
  if (t->ev_ba_read) hipEventDestroy(t->ev_ba_read);
  if (t->d_log) { hipFree(t->d_log); hipFree(t->d_log_n); hipFree(t->d_log_sink); }
  for (int l = 0; l < t->ctx->levels; l++) hipFree(t->d_pc[l]);
  hipFree(t->d_pc_ptrs); hipFree(t->d_pts); hipFree(t->d_partials); if (t->h_mail) hipHostFree(t->h_mail); if (t->h_rec) hipHostFree(t->h_rec);
  if (t->h_tot) hipHostFree(t->h_tot);
  hipFree(t->d_arrive); hipFree(t->d_leave);
  t->pipe.release();
  if (t->d_cl_part) hipFree(t->d_cl_part);
  if (t->d_cl_cnt) hipFree(t->d_cl_cnt);
  delete t;
}

int dmvio_hip_tracker_set_settings(dmvio_hip_tracker* t, const dmvio_hip_tracker_settings* s) {
  if (!t || !s) return failmsg("tracker_set_settings: null argument");
  t->dev.huberTH = s->huberTH; t->dev.coarseCutoffTH = s->coarseCutoffTH; t->dev.modeA = s->affineOptModeA; t->dev.modeB = s->affineOptModeB;
  return 0;
}

int dmvio_hip_tracker_make_k(dmvio_hip_tracker* t, const float k[4]) {
  if (!t || !k) return failmsg("tracker_make_k: null argument");
  const int L = t->ctx->levels;
  LevelGeom* g = t->dev.g;
  g[0].fx = k[0]; g[0].fy = k[1]; g[0].cx = k[2]; g[0].cy = k[3];
  for (int l = 1; l < L; l++) {
    g[l].fx = g[l - 1].fx * 0.5;
    g[l].fy = g[l - 1].fy * 0.5;
    g[l].cx = (g[0].cx + 0.5) / ((int)1 << l) - 0.5;
    g[l].cy = (g[0].cy + 0.5) / ((int)1 << l) - 0.5;
  }
  for (int l = 0; l < L; l++) {
    // K^-1 by cofactors / determinant in float (what Eigen's Matrix3f::inverse() evaluates for
    // K = [fx 0 cx; 0 fy cy; 0 0 1]; CoarseTracker.cpp:127-128)
    const float a = g[l].fx, e = g[l].fy, c = g[l].cx, f = g[l].cy;
    const float det = a * (e * 1.0f - f * 0.0f);
    const float invdet = 1.0f / det;
    float* Ki = g[l].Ki;
    Ki[0] = (e * 1.0f - f * 0.0f) * invdet; Ki[1] = (c * 0.0f - 0.0f * 1.0f) * invdet; Ki[2] = (0.0f * f - c * e) * invdet;
    Ki[3] = (f * 0.0f - 0.0f * 1.0f) * invdet; Ki[4] = (a * 1.0f - c * 0.0f) * invdet; Ki[5] = (c * 0.0f - a * f) * invdet;
    Ki[6] = (0.0f * 0.0f - e * 0.0f) * invdet; Ki[7] = (0.0f * 0.0f - a * 0.0f) * invdet; Ki[8] = (a * e - 0.0f * 0.0f) * invdet;
  }
  t->haveK = true;
  return 0;
}

// One fused calcRes + calcGSSSE evaluation, result in t->h_tot when the call returns: ONE launch, no stream synchronisation — the
// last workgroup stores the sums and then the launch's ticket into host-coherent memory and the host spins on the ticket.
// G workgroups of 256 threads split the template (point index first = rank * 256 + thread, stride G * 256) and the partial sums are
// added in rank order: with G = the cluster size of a one-problem k_track_lm launch the sums are bit-identical to the device-resident LM's.
static int evalFused(dmvio_hip_tracker* t, int lvl, int new_slot, const EvalP& e, int G) {
  dmvio_hip_ctx* c = t->ctx;
  constexpr int T = 256;
  G = std::max(1, std::min(G, t->max_eval_blocks));
  const unsigned int ticket = ++t->eval_ticket;
  hipLaunchKernelGGL(k_eval_fused<T>, dim3(G), dim3(T), 0, c->stream, t->dev, c->frames.built_on_stream(), new_slot, e, t->d_partials, t->d_arrive, t->h_tot, ticket);
  HIPCHK(hipGetLastError());
  volatile unsigned int* flag = reinterpret_cast<volatile unsigned int*>(t->h_tot) + ACC_PAD;
  unsigned long long spins = 0;
  while (*flag != ticket) {
    __builtin_ia32_pause();
    if ((++spins & 0xFFFFF) == 0) {   // every ~million polls (a few ms): has the launch failed instead of finishing?
      const hipError_t q = hipStreamQuery(c->stream);
      if (q != hipSuccess && q != hipErrorNotReady) return fail("k_eval_fused", __FILE__, __LINE__, q);
      if (q == hipSuccess && *flag != ticket) return failmsg("tracker evaluation finished without publishing its result");
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}

// ---- evaluation server session: serverStart launches k_eval_server for one frame slot, serverEval posts a request and polls the sums, serverStop tells the kernel to leave.
// The kernel also leaves by itself after 5 ms without a request (a callback that takes longer — a factor-graph solve — simply finds it gone: serverEval relaunches it).
// ticket into the mailbox: the copy in the last dword first, then the first dword (the device accepts a read only when both show the same new value)
static void mailTicket(dmvio_hip_tracker* t, unsigned int v) {
  __atomic_store_n(&t->h_mail[EVAL_MAIL_DWORDS - 1], v, __ATOMIC_RELEASE);
  __atomic_store_n(&t->h_mail[0], v, __ATOMIC_RELEASE);
}
static int serverLaunch(dmvio_hip_tracker* t) {
  dmvio_hip_ctx* c = t->ctx;
  hipLaunchKernelGGL(k_eval_server<256>, dim3(t->server_G), dim3(256), 0, c->stream, t->dev, c->frames.built_on_stream(), t->server_slot, (const unsigned int*)t->h_mail, t->d_leave, t->eval_ticket,
                     t->server_idle_ticks, t->h_rec, t->server_session);
  HIPCHK(hipGetLastError());
  return 0;
}
static int serverStart(dmvio_hip_tracker* t, int new_slot, int G) {
  t->server_G = std::max(1, std::min(G, (int)EVAL_SERVER_MAX_BLOCKS));
  t->server_slot = new_slot;
  t->eval_ticket = (t->eval_ticket + 1) & ~EVAL_QUIT_BIT;   // a number of its own for the launch
  // a session number of its own too: a workgroup of the PREVIOUS launch that has not polled its quit ticket yet (serverStop does not wait) must not take this
  // session's tickets for requests — it compares the mailbox's session dword with its own and leaves
  t->server_session++;
  __atomic_store_n(&t->h_mail[EVAL_MAIL_SESSION], t->server_session, __ATOMIC_RELEASE);
  mailTicket(t, t->eval_ticket);   // "nothing new" for the kernel about to start
  if (int r = serverLaunch(t)) return r;
  t->server_on = true;
  return 0;
}
static void serverStop(dmvio_hip_tracker* t) {
  if (!t->server_on) return;
  mailTicket(t, t->eval_ticket | EVAL_QUIT_BIT);
  t->server_on = false;
}
static int serverEval(dmvio_hip_tracker* t, const EvalP& e) {
  dmvio_hip_ctx* c = t->ctx;
  static_assert(sizeof(EvalP) / 4 + 3 <= EVAL_MAIL_DWORDS, "EvalP must fit the mailbox between the ticket and the session / ticket copy");
  const int G = t->server_G;
  auto nextTicket = [&]() { unsigned int v = (t->eval_ticket + 1) & ~EVAL_QUIT_BIT; if (v == 0) v = 1; t->eval_ticket = v; return v; };
  memcpy((void*)(t->h_mail + 1), &e, sizeof(EvalP));
  unsigned int ticket = nextTicket();
  mailTicket(t, ticket);
  // wait for the record of every workgroup (ticket behind its sums), last rank first: the others are usually there by then
  auto pending = [&]() -> bool {
    for (int g = G - 1; g >= 0; g--)
      if (reinterpret_cast<volatile unsigned int*>(t->h_rec + (size_t)g * EVAL_RECORD_FLOATS)[ACC_PAD] != ticket) return true;
    return false;
  };
  unsigned long long spins = 0;
  int restarts = 0;
  const auto t_begin = std::chrono::steady_clock::now();
  while (pending()) {
    __builtin_ia32_pause();
    if ((++spins & 0x7FFF) == 0) {   // a request takes ~12 us; every ~30 thousand polls (about a hundred microseconds) ask whether the server is still there
      if (std::chrono::steady_clock::now() - t_begin > std::chrono::seconds(5)) {   // never spin forever: report, and let the kernel leave
        mailTicket(t, t->eval_ticket | EVAL_QUIT_BIT);
        t->server_on = false;
        return failmsg("evaluation server did not answer within 5 s");
      }
      const hipError_t q = hipStreamQuery(c->stream);
      if (q != hipSuccess && q != hipErrorNotReady) return fail("k_eval_server", __FILE__, __LINE__, q);
      if (q == hipSuccess && pending()) {
        // the kernel left (idle time-out) without serving this request: start it again (it takes the mailbox's current ticket as seen) and post the request again under
        // the next number
        if (++restarts > 8) return failmsg("evaluation server keeps leaving before it serves the request");
        if (int r = serverLaunch(t)) return r;             // first_seen = eval_ticket = the unanswered ticket: nothing new for the kernel about to start ...
        ticket = nextTicket();                             // ... and the request itself under a fresh number
        mailTicket(t, ticket);
      }
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  // the sums of the evaluation: the partial sums added in rank order — ((0 + p0) + p1) + ... per slot, exactly what the device-side reductions compute
  for (int k = 0; k < ACC_PAD; k++) {
    float sacc = 0.0f;
    for (int g = 0; g < G; g++) sacc += t->h_rec[(size_t)g * EVAL_RECORD_FLOATS + k];
    t->h_tot[k] = sacc;
  }
  return 0;
}

int dmvio_hip_tracker_eval(dmvio_hip_tracker* t, int lvl, int new_slot, float new_exposure, const double pose7[7], const double aff[2],
                           float cutoffTH, double res6[6], double H[64], double b[8]) {
  if (!t || !pose7 || !aff) return failmsg("tracker_eval: null argument");
  dmvio_hip_ctx* c = t->ctx;
  if (!t->haveK || !t->haveRef) return failmsg("tracker_eval: makeK / setCoarseTrackingRef not called");
  if (lvl < 0 || lvl >= c->levels || new_slot < 0 || new_slot >= c->n_slots) return failmsg("tracker_eval: out of range");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  if (int r = dmv_ensure_row_major_locked(c, new_slot)) return r;
  EvalP e;
  makeEvalP(t->dev, lvl, poseFrom7(pose7), aff[0], aff[1], new_exposure, cutoffTH, e);
  const int n = t->dev.pc_n[lvl];
  // eval_blocks of dmvio_hip_tracker_set_launch_shape is "workgroups per fused evaluation": this call is one (it used to ignore the knob, so that no grouping but one
  // point per thread was reachable from here — the grouping the LM kernels never run at)
  if (int r = evalFused(t, lvl, new_slot, e, t->eval_blocks_override > 0 ? t->eval_blocks_override : (n + 255) / 256)) return r;
  if (res6) res6FromSums(t->h_tot, res6);
  if (H && b) systemFromSums(t->h_tot, H, b);
  return 0;
}

// ------------------------------------------------------------------ batched device-resident LM
// Entry points: argument checks, the context's lock, then a ...Locked function (the caller of those holds c->mu and has selected the device).
static int stageChecks(dmvio_hip_tracker* t, int B, const int* new_slots, const double* pose7_in, const double* aff_in, int coarsestLvl) {
  if (!t || !new_slots || !pose7_in || !aff_in) return failmsg("track_batch_stage: null argument");
  if (!t->haveK || !t->haveRef) return failmsg("track: makeK / setCoarseTrackingRef not called");
  if (B <= 0) return failmsg("track: B must be positive");
  if (coarsestLvl < 0 || coarsestLvl >= t->ctx->levels || coarsestLvl >= 5) return failmsg("track: coarsestLvl out of range");
  return 0;
}

// Cluster mode spins on a device-scope barrier, so every workgroup of such a launch must be resident at once: 256 CUs x 4 workgroups of 256 threads (k_track_lm, k_track_lm_w
// and k_track_lm_pp all keep four per CU; resource figures in DESIGN.md).  One workgroup per problem has no such limit: batches beyond the resident slots simply queue.
enum { LM_RESIDENT_WORKGROUPS = 1024 };

// the caller's arrays -> the problem records the LM kernels read (minRes NULL: no abort thresholds, NaN; new_exposures NULL: 1)
static void packProblems(LMProblemIn* in, int B, const int* new_slots, const float* new_exposures, const double* pose7_in, const double* aff_in, const double* minRes) {
  for (int i = 0; i < B; i++) {
    LMProblemIn& p = in[i];
    memcpy(p.pose7, pose7_in + 7 * i, sizeof(double) * 7);
    p.aff[0] = aff_in[2 * i]; p.aff[1] = aff_in[2 * i + 1];
    for (int k = 0; k < 5; k++) p.minRes[k] = minRes ? minRes[5 * i + k] : NAN;
    p.new_slot = new_slots[i];
    p.new_exposure = new_exposures ? new_exposures[i] : 1.0f;
  }
}
// the result records -> the caller's arrays (every one optional); returns the evaluations and point evaluations of the batch
struct LmWork { long long evals = 0, point_evals = 0; };
static LmWork unpackResults(const LMProblemOut* out, int B, double* pose7_out, double* aff_out, double* lastResiduals, double* lastFlow, double* H, double* b, int* good,
                            int* iterations) {
  LmWork w;
  for (int i = 0; i < B; i++) {
    const LMProblemOut& o = out[i];
    if (pose7_out) memcpy(pose7_out + 7 * i, o.pose7, sizeof(double) * 7);
    if (aff_out) { aff_out[2 * i] = o.aff[0]; aff_out[2 * i + 1] = o.aff[1]; }
    if (lastResiduals) memcpy(lastResiduals + 5 * i, o.lastRes, sizeof(double) * 5);
    if (lastFlow) memcpy(lastFlow + 3 * i, o.flow, sizeof(double) * 3);
    if (H) memcpy(H + 64 * i, o.H, sizeof(double) * 64);
    if (b) memcpy(b + 8 * i, o.b, sizeof(double) * 8);
    if (good) good[i] = o.good;
    if (iterations) iterations[i] = o.iterations;
    w.evals += o.n_evals; w.point_evals += o.n_point_evals;
  }
  return w;
}
// the launch argument of the k_track_lm kernels for C workgroups per problem; a cluster launch (C > 1) adds its exchange buffers
static ClusterArgs clusterArgs(int C, LMProblemOut* discard, int res_only) {
  ClusterArgs cl; cl.C = C; cl.part = nullptr; cl.cnt = nullptr; cl.discard = discard; cl.log = nullptr; cl.log_n = nullptr;
  cl.res_only = res_only;
  return cl;
}

static int stageLocked(dmvio_hip_tracker* t, int B, const int* new_slots, const float* new_exposures, const double* pose7_in, const double* aff_in, int coarsestLvl,
                       const double* minRes) {
  dmvio_hip_ctx* c = t->ctx;
  BatchPipeline& pl = t->pipe;
  if (int r = pl.reserve(B, c->stream)) return r;
  int half;
  if (int r = pl.stageInto(&half)) return r;
  for (int i = 0; i < B; i++) if (new_slots[i] < 0 || new_slots[i] >= c->n_slots) return failmsg("track: frame slot out of range");
  packProblems(pl.in(half), B, new_slots, new_exposures, pose7_in, aff_in, minRes);
  pl.stageDone(half, B, coarsestLvl);
  return 0;
}

int dmvio_hip_tracker_track_batch_stage(dmvio_hip_tracker* t, int B, const int* new_slots, const float* new_exposures,
                                        const double* pose7_in, const double* aff_in, int coarsestLvl, const double* minRes) {
  if (int r = stageChecks(t, B, new_slots, pose7_in, aff_in, coarsestLvl)) return r;
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  HIPCHK(hipSetDevice(t->ctx->device));
  return stageLocked(t, B, new_slots, new_exposures, pose7_in, aff_in, coarsestLvl, minRes);
}

// Workgroups per alignment problem.  The evaluation time falls with 1/C while every evaluation pays one device-scope barrier whose cost
// grows with the number of workgroups in flight, so the best C grows with the template (about sqrt(points)) and shrinks with the batch;
// the table is the argmin of a measured sweep (tools/sweep_tracking.py --cluster, profiles/r01_tracking_sweep.md) over
// template size (level-0 points) x batch size.
static int clusterSize(const int B, const int pc0) {
  if (B > 128) return 1;
  const int sz = pc0 < 20000 ? 0 : (pc0 < 70000 ? 1 : (pc0 < 180000 ? 2 : 3));
  const int bb = B <= 4 ? 0 : (B <= 8 ? 1 : (B <= 16 ? 2 : (B <= 32 ? 3 : (B <= 64 ? 4 : 5))));
  static const int tab[4][6] = {{8, 8, 4, 4, 4, 1}, {8, 8, 8, 4, 4, 4}, {32, 16, 8, 8, 4, 4}, {32, 16, 16, 8, 8, 4}};   // re-measured in round 2 (profiles/r02_tracking_cluster_sweep.md)
  return tab[sz][bb];
}

// The instantiations of the batch kernels a launch can reach (every k_track_lm with four tap sets in flight), and the one table of which shape has one.
enum LmKernel { LM_NONE, LM_256_TILED, LM_512_TILED, LM_1024, LM_512, LM_256, LM_PP };
struct LmVariant { int T; bool tiled, cluster; LmKernel k; };   // cluster: also runs with C > 1 workgroups per problem
static const LmVariant kLmVariants[] = {{256, true, true, LM_256_TILED}, {512, true, false, LM_512_TILED}, {1024, false, false, LM_1024}, {512, false, false, LM_512},
                                        {256, false, true, LM_256}};
static LmKernel lmVariant(int T, int C, bool tiled) {
  for (const LmVariant& v : kLmVariants) if (v.T == T && v.tiled == tiled && (C == 1 || v.cluster)) return v.k;
  return LM_NONE;
}

struct LaunchShape {
  int C = 1, T = 0;              // workgroups per problem, threads per workgroup
  bool tiled = false;            // the kernel gathers level 0 from 8x4 tiles where a problem's slot has them (decided per problem inside the kernel)
  bool untile = false;           // some slots are tiled and the shape has no tiled variant: convert the batch's slots back before the launch
  LmKernel kernel = LM_NONE;
  const char* refusal = nullptr;
};
// Launch shape of a batch of B problems on a template of pc0 level-0 points.  Pure: reads nothing but its arguments.
// Up to 128 problems -> cluster mode: C workgroups of 256 threads per problem (latency; measured on MI355X: B=1 240 us with C=8 vs
// 367 us for one 1024-thread workgroup); more -> one workgroup per problem (512 threads up to 512 problems, then 256 threads,
// four resident per CU: throughput).
// Overridable for experiments: dmvio_hip_tracker_set_launch_shape (lm_threads / lm_cluster; 0 = the choice above).
static LaunchShape chooseLaunchShape(int B, int pc0, int lm_threads, int lm_cluster, bool want_pp, bool any_tiled) {
  LaunchShape s;
  if (lm_cluster > 0) s.C = lm_cluster;
  else if (!lm_threads) s.C = clusterSize(B, pc0);
  if (s.C > 1 && (long)B * s.C > LM_RESIDENT_WORKGROUPS) { s.refusal = "track_batch_launch: cluster size too large for the batch (B*C must be <= 1024 resident workgroups)"; return s; }
  // threads per workgroup: 256 in cluster mode and for full batches (four workgroups per CU); batches that cannot fill the CUs that way
  // (129..512 problems) take 512 threads per problem (measured: B=256 0.47 -> 0.40 ms, B=512 0.62 -> 0.58 ms)
  s.T = lm_threads ? lm_threads : (s.C > 1 ? 256 : (B <= 128 ? 1024 : (B <= 512 ? 512 : 256)));
  // frames whose level 0 the batched raw-image build stored in 8x4 tiles: the 256- and 512-thread configurations have an instantiation that gathers from them
  // directly; any other configuration has those slots converted back first
  s.tiled = any_tiled && lmVariant(s.T, s.C, true) != LM_NONE;
  s.untile = any_tiled && !s.tiled;
  s.kernel = lmVariant(s.T, s.C, s.tiled);
  if (s.kernel == LM_NONE) s.refusal = "track_batch_launch: lm_threads (dmvio_hip_tracker_set_launch_shape) must be 128/256/512/1024 (cluster mode: 256)";
  // full batches: five-wave workgroups holding two problems each, the LM control step of one beside the evaluation of the other; persistent grid, problems dealt out by a
  // device-wide counter
  else if (want_pp && s.kernel == LM_256 && s.C == 1 && B >= 512) s.kernel = LM_PP;
  return s;
}

static int launchLocked(dmvio_hip_tracker* t) {
  BatchPipeline& pl = t->pipe;
  if (pl.staged_B <= 0) return failmsg("track_batch_launch: nothing staged");
  dmvio_hip_ctx* c = t->ctx;
  const int B = pl.staged_B;
  pl.unlaunched = false;
  // (the context's lock is held from the scan of the layout flags to the launch: a batched raw-image build on another thread — dmvio_hip_set_build_stream invites one — must
  // not flip a slot's layout between the choice of the instantiation and the launch that relies on it)
  const LMProblemIn* pin = pl.in(pl.staged_half);
  bool any_tiled = false;
  for (int i = 0; i < B && !any_tiled; i++) any_tiled = c->frames.is_tiled(pin[i].new_slot);
  const LaunchShape s = chooseLaunchShape(B, t->dev.pc_n[0], t->lm_threads_override, t->lm_cluster_override, t->batch_kernel == 1 && !t->debug_mode, any_tiled);
  if (s.refusal) return failmsg(s.refusal);
  const int C = s.C;
  ClusterArgs cl = clusterArgs(C, pl.d_discard, t->res_only_evals);
  // Slots a deferred attach left without their coarser levels (dmvio_hip_frames_attach_device_batch): full batches on the plain 256-thread kernel go to k_track_lm_build,
  // whose workgroups build their own frame's pyramid first, where the store lets the launch claim them (FrameSlots::claimWaiting_locked: the launch below is the next thing on
  // the stream and this thread holds the context's lock until then).  Every other launch has them built by the ordinary kernel first, on this stream.
  t->last_fused_builds = 0;
  const int fused = s.kernel == LM_256 && C == 1 && !t->debug_mode ? c->frames.claimWaiting_locked(B, [pin](int i) { return pin[i].new_slot; }) : c->frames.flush(false);
  if (fused < 0) return fused;
  if (t->debug_mode) {
    // diagnostics: 1 = record the evaluations of this launch, 2 = run the recorded evaluations again without the control steps (dmvio_hip_tracker_debug_record_replay)
    if (C != 1 || s.T != 256) return failmsg("tracker record / replay: full batches only (one 256-thread workgroup per problem)");
    if (B > t->log_cap) {
      if (t->d_log) { HIPCHK(hipFree(t->d_log)); HIPCHK(hipFree(t->d_log_n)); HIPCHK(hipFree(t->d_log_sink)); }
      HIPCHK(hipMalloc((void**)&t->d_log, sizeof(EvalP) * (size_t)B * LM_LOG_EVALS)); HIPCHK(hipMalloc((void**)&t->d_log_n, sizeof(int) * B));
      HIPCHK(hipMalloc((void**)&t->d_log_sink, sizeof(float) * (size_t)B * ACC_PAD));
      t->log_cap = B; t->log_B = 0;
    }
    if (t->debug_mode == 1) { cl.log = t->d_log; cl.log_n = t->d_log_n; t->log_B = B; }
    else {
      if (t->log_B != B) return failmsg("tracker replay: record a launch of the same batch first");
      hipLaunchKernelGGL((k_track_replay<256, 4>), dim3(B), dim3(256), 0, c->stream, t->dev, c->frames.as_is(), pin, (const EvalP*)t->d_log, (const int*)t->d_log_n, t->d_log_sink);
      HIPCHK(hipGetLastError());
      return 0;   // nothing to fetch: the caller times the launch and synchronises the stream itself
    }
  }
  t->last.cluster = C; t->last.threads = s.T;
  if (C > 1) {
    const size_t need = (size_t)B * 2 * C * ACC_PAD;
    if (need > t->cl_part_cap) { if (t->d_cl_part) HIPCHK(hipFree(t->d_cl_part)); HIPCHK(hipMalloc((void**)&t->d_cl_part, sizeof(float) * need)); t->cl_part_cap = need; }
    if (B > t->cl_cnt_cap) { if (t->d_cl_cnt) HIPCHK(hipFree(t->d_cl_cnt)); HIPCHK(hipMalloc((void**)&t->d_cl_cnt, sizeof(unsigned int) * B)); t->cl_cnt_cap = B; }
    HIPCHK(hipMemsetAsync(t->d_cl_cnt, 0, sizeof(unsigned int) * B, c->stream));
    cl.part = t->d_cl_part; cl.cnt = t->d_cl_cnt;
  }
  if (s.untile)
    for (int i = 0; i < B; i++) if (int r = dmv_ensure_row_major_locked(c, pin[i].new_slot)) return r;
  LMProblemOut* pout = pl.out(pl.staged_half);
  auto lm = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(B * C), dim3(s.T), 0, c->stream, t->dev, c->frames.as_is(), pin, pout, pl.staged_coarsest, cl); };
  switch (s.kernel) {
    case LM_256_TILED: lm(k_track_lm<256, 4, true>); break;
    case LM_512_TILED: lm(k_track_lm<512, 4, true>); break;
    case LM_1024: lm(k_track_lm<1024, 4, false>); break;
    case LM_512: lm(k_track_lm<512, 4, false>); break;
    case LM_256:
      if (fused) {
        hipLaunchKernelGGL((k_track_lm_build<256, 4>), dim3(B), dim3(256), 0, c->stream, t->dev, c->frames.as_is(), pin, pout, pl.staged_coarsest, cl, c->pg);
        t->last_fused_builds = fused;
      } else lm(k_track_lm<256, 4, false>);
      break;
    case LM_PP: {
      if (!t->d_pp_next) HIPCHK(hipMalloc((void**)&t->d_pp_next, sizeof(unsigned int)));
      HIPCHK(hipMemsetAsync(t->d_pp_next, 0, sizeof(unsigned int), c->stream));
      const int grid = std::min((B + 1) / 2, (int)LM_RESIDENT_WORKGROUPS);   // persistent: no more workgroups than are resident at 128 registers
      hipLaunchKernelGGL(k_track_lm_pp, dim3(grid), dim3(256), 0, c->stream, t->dev, c->frames.as_is(), pin, pout, pl.staged_coarsest, B, t->d_pp_next);
      break;
    }
    case LM_NONE: break;   // refused above
  }
  HIPCHK(hipGetLastError());
  return pl.launched(c->stream);
}

// Problems of the last batch launch whose frame's pyramid the tracking kernel formed itself (a deferred attach, dmvio_hip_set_deferred_attach); 0: the launch found every
// slot built, or was one that has the waiting slots built first.
int dmvio_hip_tracker_last_fused_builds(dmvio_hip_tracker* t) {
  if (!t) return failmsg("tracker_last_fused_builds: null tracker");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  return t->last_fused_builds;
}

int dmvio_hip_tracker_track_batch_launch(dmvio_hip_tracker* t) {
  if (!t) return failmsg("track_batch_launch: nothing staged");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  HIPCHK(hipSetDevice(t->ctx->device));
  return launchLocked(t);
}

// Marks the results of the last launch as "to be fetched later": the caller may queue the NEXT batch (pyramids, stage, launch) before
// blocking in _fetch, so the device never waits for the host to unpack results.
int dmvio_hip_tracker_track_batch_fetch_begin(dmvio_hip_tracker* t) {
  if (!t || t->pipe.staged_B <= 0) return failmsg("track_batch_fetch_begin: nothing staged");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  HIPCHK(hipSetDevice(t->ctx->device));
  t->pipe.fetchBegin();
  return 0;
}

static int fetchLocked(dmvio_hip_tracker* t, double* pose7_out, double* aff_out, double* lastResiduals, double* lastFlow, double* H, double* b, int* good, int* iterations) {
  if (t->pipe.staged_B <= 0) return failmsg("track_batch_fetch: nothing staged");
  int B, half;
  if (int r = t->pipe.take(&half, &B)) return r;
  const LMProblemOut* out = t->pipe.out(half);
  LastRun run;
  run.cluster = t->last.cluster; run.threads = t->last.threads; run.vio_iterations = t->last.vio_iterations;   // those belong to the launch / the last host-LM call
  run.repeat_lvl = std::move(t->last.repeat_lvl); run.first_pass_res = std::move(t->last.first_pass_res);     // (their storage, not their contents)
  run.repeat_lvl.resize(B); run.first_pass_res.resize(B);
  const LmWork work = unpackResults(out, B, pose7_out, aff_out, lastResiduals, lastFlow, H, b, good, iterations);
  run.evals = work.evals; run.point_evals = work.point_evals;
  for (int i = 0; i < B; i++) {
    const LMProblemOut& o = out[i];
    run.repeat_lvl[i] = o.repeated_lvl; run.first_pass_res[i] = o.first_pass_res;
    run.ticks_step += o.ticks_step; run.ticks_eval += o.ticks_eval;
    run.res_evals += o.n_res_evals; run.res_point_evals += o.n_res_point_evals;
  }
  t->last = std::move(run);
  return 0;
}

int dmvio_hip_tracker_track_batch_fetch(dmvio_hip_tracker* t, double* pose7_out, double* aff_out, double* lastResiduals, double* lastFlow,
                                        double* H, double* b, int* good, int* iterations) {
  if (!t) return failmsg("track_batch_fetch: nothing staged");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  HIPCHK(hipSetDevice(t->ctx->device));
  return fetchLocked(t, pose7_out, aff_out, lastResiduals, lastFlow, H, b, good, iterations);
}

static int vioChecks(dmvio_hip_tracker* t, int new_slot, const double* pose7_io, const double* aff_io, int coarsestLvl);
static int trackVioLocked(dmvio_hip_tracker* t, int new_slot, float new_exposure, double pose7_io[7], double aff_io[2], int coarsestLvl, const double minResForAbort[5],
                          const dmvio_hip_coarse_callbacks* cb, double lastResiduals[5], double lastFlow[3], double H_out[64], double b_out[8], int* good, int* n_evals);

// dmvio_hip_tracker_track_batch.  allow_host_lm = false: never the single-problem shortcut below (a rank's share of trackNewCoarse's hypotheses runs the device-resident LM
// like the batch of the unsplit call does, even when the share is ONE try).
static int trackBatch(dmvio_hip_tracker* t, int B, const int* new_slots, const float* new_exposures, double* pose7_io, double* aff_io, int coarsestLvl, const double* minRes,
                      double* lastResiduals, double* lastFlow, double* H, double* b, int* good, int* iterations, bool allow_host_lm) {
  if (!t) return failmsg("track_batch_stage: null argument");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  HIPCHK(hipSetDevice(t->ctx->device));
  // ONE alignment problem: the LM control step (8x8 pivoted LDL^T, SE3 exp: one dependent chain) takes 6.5 us per iteration on a wavefront and well under a microsecond on
  // the host, so the loop runs on the host against the evaluation server (one launch per frame, requests through host-coherent memory).  Same split of the template and
  // same order of the partial sums as the device-resident LM's cluster mode, same arithmetic in the step: identical sums, residuals, H, b and iteration counts, the pose
  // to the last bit or two of its fp64 components (tests/test_vio_gpu.py, tests/test_edge_gpu.py); 0.165 instead of 0.25 ms per frame.
  // (not while a staged batch waits for its launch: the single-frame path would run in front of it and the caller's later _launch would find nothing)
  if (B == 1 && allow_host_lm && t->single_host_lm && t->use_server && !t->lm_threads_override && !t->lm_cluster_override && t->pipe.fetch_B == 0 && !t->pipe.unlaunched &&
      new_slots && pose7_io && aff_io) {
    if (int r = vioChecks(t, new_slots[0], pose7_io, aff_io, coarsestLvl)) return r;
    int g = 0, ne = 0;
    const float ex = new_exposures ? new_exposures[0] : 1.0f;
    if (int r = trackVioLocked(t, new_slots[0], ex, pose7_io, aff_io, coarsestLvl, minRes, nullptr, lastResiduals, lastFlow, H, b, &g, &ne)) return r;
    if (good) good[0] = g;
    if (iterations) iterations[0] = t->last.vio_iterations;
    return 0;
  }
  if (int r = stageChecks(t, B, new_slots, pose7_io, aff_io, coarsestLvl)) return r;
  if (int r = stageLocked(t, B, new_slots, new_exposures, pose7_io, aff_io, coarsestLvl, minRes)) return r;
  if (int r = launchLocked(t)) return r;
  return fetchLocked(t, pose7_io, aff_io, lastResiduals, lastFlow, H, b, good, iterations);
}

int dmvio_hip_tracker_track_batch(dmvio_hip_tracker* t, int B, const int* new_slots, const float* new_exposures, double* pose7_io, double* aff_io,
                                  int coarsestLvl, const double* minRes, double* lastResiduals, double* lastFlow, double* H, double* b,
                                  int* good, int* iterations) {
  return trackBatch(t, B, new_slots, new_exposures, pose7_io, aff_io, coarsestLvl, minRes, lastResiduals, lastFlow, H, b, good, iterations, true);
}

int dmvio_hip_tracker_track(dmvio_hip_tracker* t, int new_slot, float new_exposure, double pose7_io[7], double aff_io[2], int coarsestLvl,
                            const double minRes[5], double lastResiduals[5], double lastFlow[3], double H[64], double b[8], int* good) {
  return trackBatch(t, 1, &new_slot, &new_exposure, pose7_io, aff_io, coarsestLvl, minRes, lastResiduals, lastFlow, H, b, good, nullptr, true);
}

// The visual-only LM step of CoarseTracker.cpp:639-682 on the host: damped H, the 6 / 7 / 8-dof LDL^T variants selected by
// affineOptModeA / B, extrapolation, SCALE_* scaling, SE3::exp(inc) * refToNew_current.  This is what the reference itself executes
// while the IMU is not initialised (CoarseTracker.cpp:612: !imuIntegration.isCoarseInitialized()), and the default update of
// dmvio_hip_tracker_track_vio.  incA / incB are returned UNSCALED like computeCoarseUpdate's (the caller applies SCALE_A / SCALE_B, :633-637).
int dmvio_hip_coarse_update_visual(const dmvio_hip_tracker_settings* st, const double H[64], const double b[8], float extrapFac, float lambda,
                                   const double pose7_cur[7], double pose7_new[7], double* incA, double* incB, double* incNorm) {
  if (!H || !b || !pose7_cur || !pose7_new) return failmsg("coarse_update_visual: null argument");
  const float modeA = st ? st->affineOptModeA : 1e12f, modeB = st ? st->affineOptModeB : 1e8f;
  double Hl[64];
  memcpy(Hl, H, sizeof(Hl));
  for (int i = 0; i < 8; i++) Hl[i * 9] *= (1 + lambda);
  double inc[8];
  const bool fixA = modeA < 0, fixB = modeB < 0;
  if (!fixA && !fixB) {
    double m[64]; memcpy(m, Hl, sizeof(m));
    for (int i = 0; i < 8; i++) inc[i] = -b[i];
    ldltSolveInPlace<8>(m, 8, inc, 8);
  } else if (fixA && fixB) {
    double m[64]; memcpy(m, Hl, sizeof(m));
    for (int i = 0; i < 6; i++) inc[i] = -b[i];
    ldltSolveInPlace<8>(m, 8, inc, 6);
    inc[6] = inc[7] = 0;
  } else if (!fixA && fixB) {
    double m[64]; memcpy(m, Hl, sizeof(m));
    for (int i = 0; i < 7; i++) inc[i] = -b[i];
    ldltSolveInPlace<8>(m, 8, inc, 7);
    inc[7] = 0;
  } else {   // fix a: b's row / column take the place of a's (CoarseTracker.cpp:653-664)
    double m[64]; memcpy(m, Hl, sizeof(m));
    double bs[8]; memcpy(bs, b, sizeof(bs));
    for (int r = 0; r < 8; r++) m[r * 8 + 6] = m[r * 8 + 7];
    for (int cc = 0; cc < 8; cc++) m[6 * 8 + cc] = m[7 * 8 + cc];
    bs[6] = bs[7];
    double x[8];
    for (int i = 0; i < 7; i++) x[i] = -bs[i];
    ldltSolveInPlace<8>(m, 8, x, 7);
    for (int i = 0; i < 6; i++) inc[i] = x[i];
    inc[6] = 0; inc[7] = x[6];
  }
  for (int i = 0; i < 8; i++) inc[i] *= extrapFac;
  double incScaled[8];
  for (int i = 0; i < 6; i++) incScaled[i] = inc[i] * 1.0f;   // SCALE_XI_ROT / SCALE_XI_TRANS
  incScaled[6] = inc[6] * 10.0f; incScaled[7] = inc[7] * 1000.0f;
  double ssum = 0;
  for (int i = 0; i < 8; i++) ssum += incScaled[i];
  if (!std::isfinite(ssum)) for (int i = 0; i < 8; i++) incScaled[i] = 0;
  const Pose nxt = poseMul(poseExp(incScaled), poseFrom7(pose7_cur));
  poseTo7(nxt, pose7_new);
  // the reference's two branches differ here: the LDLT branch adds incScaled[6..7] to the affine parameters, the IMU branch receives
  // the unscaled increments and scales them itself — both give the same numbers as long as incScaled was not zeroed for being non-finite
  if (incA) *incA = std::isfinite(ssum) ? inc[6] : 0.0;
  if (incB) *incB = std::isfinite(ssum) ? inc[7] : 0.0;
  double nn = 0;
  for (int i = 0; i < 8; i++) nn += inc[i] * inc[i];
  if (incNorm) *incNorm = sqrt(nn);
  return 0;
}

// ONE alignment problem (dmvio_hip_tracker_track, a track_batch of one): 1 (default) = the host LM against the evaluation server, 0 = the device-resident LM in cluster mode
int dmvio_hip_tracker_set_single_frame_mode(dmvio_hip_tracker* t, int host_lm) {
  if (!t) return failmsg("null tracker");
  t->single_host_lm = host_lm ? 1 : 0;
  return 0;
}
// Measurement knobs (tools/sweep_tracking.py, profiles/): explicit calls instead of environment variables read behind the caller's back.  0 = the library's own choice.
//   eval_blocks: workgroups per fused evaluation / evaluation server (changes how the fp32 partial sums are grouped)
//   lm_threads: threads per workgroup of k_track_lm (256, 512 or 1024)
//   lm_waves: accepted (0, 1, 2 or 4) and without effect: every instantiation of k_track_lm that is built keeps four tap sets in flight
//   lm_cluster: workgroups that share one alignment problem in cluster mode (2 .. 32; changes the grouping of the sums)
int dmvio_hip_tracker_set_launch_shape(dmvio_hip_tracker* t, int eval_blocks, int lm_threads, int lm_waves, int lm_cluster) {
  if (!t) return failmsg("null tracker");
  if (eval_blocks < 0 || eval_blocks > t->max_eval_blocks) return failmsg("tracker_set_launch_shape: eval_blocks out of range");
  if (lm_threads != 0 && lm_threads != 256 && lm_threads != 512 && lm_threads != 1024) return failmsg("tracker_set_launch_shape: lm_threads is 0, 256, 512 or 1024");
  if (lm_waves != 0 && lm_waves != 1 && lm_waves != 2 && lm_waves != 4) return failmsg("tracker_set_launch_shape: lm_waves is 0, 1, 2 or 4");
  if (lm_cluster < 0 || lm_cluster > 32) return failmsg("tracker_set_launch_shape: lm_cluster out of range");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  t->eval_blocks_override = eval_blocks; t->lm_threads_override = lm_threads; t->lm_cluster_override = lm_cluster;
  return 0;
}
// Diagnostics for profiles/: mode 1 = the next dmvio_hip_tracker_track_batch_launch calls record the parameters of every evaluation they run (full batches: one 256-thread
// workgroup per problem), mode 2 = they run the recorded evaluations again WITHOUT the LM control steps between them (k_track_replay: same points, same taps, same fused
// sums; nothing to fetch — time the launch on the context's stream), 0 = normal operation.
int dmvio_hip_tracker_debug_record_replay(dmvio_hip_tracker* t, int mode) {
  if (!t || mode < 0 || mode > 2) return failmsg("tracker_debug_record_replay: bad argument");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  t->debug_mode = mode;
  return 0;
}
// Kernel of FULL batches (>= 512 problems, one 256-thread evaluation group per problem): 0 = k_track_lm (four wavefronts per problem: they evaluate, then three wait
// while the first solves), 1 = k_track_lm_pp (a four-wavefront workgroup holds two problems: wavefront 0 runs the control step of one, then joins the evaluation of the other; per problem the same
// arithmetic in the same order — identical results).
int dmvio_hip_tracker_set_batch_kernel(dmvio_hip_tracker* t, int mode) {
  if (!t || mode < 0 || mode > 1) return failmsg("tracker_set_batch_kernel: 0 or 1");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  t->batch_kernel = mode;
  return 0;
}
// 1 (default): k_track_lm runs an iteration step that is known to be its level's last (above level 0) as a residual-only evaluation — the seven statistics that decide
// accept / reject and lastResiduals, without the 9x9 sums, which no one reads (tracker_kernels.hpp: lmWaveStep, blockEvalRes); 0: every evaluation in full.  Every output is
// the same bit for bit either way.  k_track_lm_pp and the host-driven LM (their callbacks read H at every iteration) always evaluate in full.
int dmvio_hip_tracker_set_residual_only_evals(dmvio_hip_tracker* t, int on) {
  if (!t) return failmsg("null tracker");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  t->res_only_evals = on ? 1 : 0;
  return 0;
}
// 1 (default): the evaluations of a host-driven LM go to the resident evaluation server (one launch per tracked frame); 0: one fused launch per evaluation
int dmvio_hip_tracker_set_eval_server(dmvio_hip_tracker* t, int on) {
  if (!t) return failmsg("null tracker");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  t->use_server = on ? 1 : 0;
  return 0;
}

// How long the evaluation server of a single-frame track / track_vio call stays resident without a request (default 5000 us).  A computeCoarseUpdate hook that regularly
// takes longer (a factor-graph solve) would otherwise pay a relaunch of the kernel per LM iteration.
int dmvio_hip_tracker_set_server_idle_us(dmvio_hip_tracker* t, int microseconds) {
  if (!t || microseconds < 100 || microseconds > 2000000) return failmsg("tracker_set_server_idle_us: 100 us .. 2 s");
  t->server_idle_ticks = (long long)microseconds * 100;   // wall_clock64 runs at 100 MHz
  return 0;
}

static int vioChecks(dmvio_hip_tracker* t, int new_slot, const double* pose7_io, const double* aff_io, int coarsestLvl) {
  if (!t || !pose7_io || !aff_io) return failmsg("track_vio: null argument");
  dmvio_hip_ctx* c = t->ctx;
  if (!t->haveK || !t->haveRef) return failmsg("track_vio: makeK / setCoarseTrackingRef not called");
  if (coarsestLvl < 0 || coarsestLvl >= c->levels || coarsestLvl >= 5) return failmsg("track_vio: coarsestLvl out of range");
  if (new_slot < 0 || new_slot >= c->n_slots) return failmsg("track_vio: frame slot out of range");
  return 0;
}

// CoarseTracker::trackNewestCoarse with the LM step handed to the caller (CoarseTracker.cpp:539-770, the setting_useIMU branch
// :612-637): the host loop of the reference over device evaluations.  Every iteration costs one request to the evaluation server (or one
// fused launch) whose result the host picks up by polling host-coherent memory, plus the callback.  The callbacks run under the context's lock.
static int trackVioLocked(dmvio_hip_tracker* t, int new_slot, float new_exposure, double pose7_io[7], double aff_io[2], int coarsestLvl, const double minResForAbort[5],
                          const dmvio_hip_coarse_callbacks* cb, double lastResiduals[5], double lastFlow[3], double H_out[64], double b_out[8], int* good, int* n_evals) {
  dmvio_hip_ctx* c = t->ctx;
  if (int r = dmv_ensure_row_major_locked(c, new_slot)) return r;   // the evaluation server reads row-major planes
  const TrackerDev& trk = t->dev;
  const int G = t->eval_blocks_override > 0 ? t->eval_blocks_override : clusterSize(1, trk.pc_n[0]);
  dmvio_hip_tracker_settings st; st.huberTH = trk.huberTH; st.coarseCutoffTH = trk.coarseCutoffTH; st.affineOptModeA = trk.modeA; st.affineOptModeB = trk.modeB;
  double lastRes[5], flow[3] = {1000, 1000, 1000};
  for (int i = 0; i < 5; i++) lastRes[i] = NAN;
  const int maxIterations[5] = {10, 20, 50, 50, 50};
  const float lambdaExtrapolationLimit = 0.001f;
  Pose cur = poseFrom7(pose7_io);
  double affA = aff_io[0], affB = aff_io[1];
  bool haveRepeated = false, failed = false;
  double H[64] = {0}, b[8] = {0};
  int lastLvl = -1, evals = 0, totalIts = 0, repeatedLvl = -1;
  double firstPassRes = NAN;
  EvalP e;
  // one server launch for the whole call (requests through the mailbox) or one fused launch per evaluation
  struct Session {
    dmvio_hip_tracker* t; bool on;
    ~Session() { if (on) serverStop(t); }
  } session{t, false};
  if (t->use_server) { if (int r = serverStart(t, new_slot, G)) return r; session.on = true; }
  long long point_evals = 0;   // sum over evaluations of pc_n[lvl]: the unit count behind the roofline's algorithmic bytes (dmvio_hip_tracker_last_work)
  auto evaluate = [&](const EvalP& ep, int lv) -> int { point_evals += trk.pc_n[lv]; return session.on ? serverEval(t, ep) : evalFused(t, lv, new_slot, ep, G); };
  for (int lvl = coarsestLvl; lvl >= 0 && !failed; lvl--) {
    float levelCutoffRepeat = 1;
    double resOld[6];
    makeEvalP(trk, lvl, cur, affA, affB, new_exposure, trk.coarseCutoffTH * levelCutoffRepeat, e);
    if (int r = evaluate(e, lvl)) return r;
    evals++;
    res6FromSums(t->h_tot, resOld);
    while (resOld[5] > 0.6 && (levelCutoffRepeat < 50 || resOld[5] > 0.99)) {
      levelCutoffRepeat *= 2;
      makeEvalP(trk, lvl, cur, affA, affB, new_exposure, trk.coarseCutoffTH * levelCutoffRepeat, e);
      if (int r = evaluate(e, lvl)) return r;
      evals++;
      res6FromSums(t->h_tot, resOld);
    }
    systemFromSums(t->h_tot, H, b);
    float lambda = 0.01f;
    for (int iteration = 0; iteration < maxIterations[lvl]; iteration++) {
      float extrapFac = 1;
      if (lambda < lambdaExtrapolationLimit) extrapFac = sqrtf(sqrtf(lambdaExtrapolationLimit / lambda));
      double cur7[7], nxt7[7], incA = 0, incB = 0, incNorm = 0;
      poseTo7(cur, cur7);
      int rc;
      if (cb && cb->update) {
        const double affc[2] = {affA, affB};
        rc = cb->update(cb->user, H, b, extrapFac, lambda, cur7, affc, nxt7, &incA, &incB, &incNorm);
        if (rc) return failmsg("track_vio: the coarse-update callback reported an error");
      } else if ((rc = dmvio_hip_coarse_update_visual(&st, H, b, extrapFac, lambda, cur7, nxt7, &incA, &incB, &incNorm))) return rc;
      const Pose nxt = poseFrom7(nxt7);
      const double affA_n = affA + incA * 10.0f, affB_n = affB + incB * 1000.0f;   // SCALE_A, SCALE_B (CoarseTracker.cpp:633-637)
      makeEvalP(trk, lvl, nxt, affA_n, affB_n, new_exposure, trk.coarseCutoffTH * levelCutoffRepeat, e);
      if (int r = evaluate(e, lvl)) return r;
      evals++;
      double resNew[6];
      res6FromSums(t->h_tot, resNew);
      const bool accept = (resNew[0] / resNew[1]) < (resOld[0] / resOld[1]);
      if (accept) {
        systemFromSums(t->h_tot, H, b);
        for (int i = 0; i < 6; i++) resOld[i] = resNew[i];
        affA = affA_n; affB = affB_n; cur = nxt;
        if (cb && cb->accept) cb->accept(cb->user);
        lambda *= 0.5f;
      } else {
        lambda *= 4;
        if (lambda < lambdaExtrapolationLimit) lambda = lambdaExtrapolationLimit;
      }
      lastLvl = lvl;
      totalIts++;
      if (!(incNorm > 1e-3)) break;
    }
    lastRes[lvl] = sqrtf((float)(resOld[0] / resOld[1]));
    flow[0] = resOld[2]; flow[1] = resOld[3]; flow[2] = resOld[4];
    if (std::isnan(lastRes[lvl]) || (minResForAbort && lastRes[lvl] > 1.5 * minResForAbort[lvl])) { failed = true; break; }
    if (levelCutoffRepeat > 1 && !haveRepeated) { repeatedLvl = lvl; firstPassRes = lastRes[lvl]; lvl++; haveRepeated = true; }
  }
  // bookkeeping of the "last launch" queries: this call's own numbers, not those of an earlier batch
  LastRun run;
  run.cluster = session.on ? t->server_G : G; run.threads = 256;
  run.evals = evals; run.point_evals = point_evals; run.vio_iterations = totalIts;
  run.repeat_lvl.assign(1, repeatedLvl); run.first_pass_res.assign(1, firstPassRes);
  t->last = std::move(run);
  if (lastResiduals) memcpy(lastResiduals, lastRes, sizeof(lastRes));
  if (lastFlow) memcpy(lastFlow, flow, sizeof(flow));
  if (n_evals) *n_evals = evals;
  if (H_out) memcpy(H_out, H, sizeof(H));
  if (b_out) memcpy(b_out, b, sizeof(b));
  if (failed) { if (good) *good = 0; return 0; }   // the reference returns false without touching lastToNew_out / aff_g2l_out (:731-732)
  double aff[2] = {affA, affB};
  bool trackingGood = true;
  if ((trk.modeA != 0 && (fabsf((float)aff[0]) > 1.2f)) || (trk.modeB != 0 && (fabsf((float)aff[1]) > 200.0f))) trackingGood = false;
  double rel[2];
  affFromTo(trk.ref_exposure, new_exposure, trk.ref_aff_a, trk.ref_aff_b, aff[0], aff[1], rel);
  if ((trk.modeA == 0 && (fabsf(logf((float)rel[0])) > 1.5f)) || (trk.modeB == 0 && (fabsf((float)rel[1]) > 200.0f))) trackingGood = false;
  if (trk.modeA < 0) aff[0] = 0;
  if (trk.modeB < 0) aff[1] = 0;
  poseTo7(cur, pose7_io);
  aff_io[0] = aff[0]; aff_io[1] = aff[1];
  if (good) *good = trackingGood ? 1 : 0;
  if (lastLvl == 0 && cb && cb->visual) cb->visual(cb->user, H, b, trackingGood ? 1 : 0);   // addVisualToCoarseGraph (:763-767)
  return 0;
}

int dmvio_hip_tracker_track_vio(dmvio_hip_tracker* t, int new_slot, float new_exposure, double pose7_io[7], double aff_io[2], int coarsestLvl,
                                const double minResForAbort[5], const dmvio_hip_coarse_callbacks* cb, double lastResiduals[5], double lastFlow[3],
                                double H_out[64], double b_out[8], int* good, int* n_evals) {
  if (int r = vioChecks(t, new_slot, pose7_io, aff_io, coarsestLvl)) return r;
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  HIPCHK(hipSetDevice(t->ctx->device));
  return trackVioLocked(t, new_slot, new_exposure, pose7_io, aff_io, coarsestLvl, minResForAbort, cb, lastResiduals, lastFlow, H_out, b_out, good, n_evals);
}

// lastF_2_fh_tries of FullSystem::trackNewCoarse (FullSystem.cpp:364-402) from three camToWorld poses
int dmvio_hip_make_track_hypotheses(const double slast_c2w[7], const double sprelast_c2w[7], const double lastF_c2w[7], double* out, int max_out) {
  if (!slast_c2w || !sprelast_c2w || !lastF_c2w || !out) return failmsg("make_track_hypotheses: null argument");
  const Pose slast = poseFrom7(slast_c2w), sprelast = poseFrom7(sprelast_c2w), lastF = poseFrom7(lastF_c2w);
  const Pose fh_2_slast = poseMul(poseInv(sprelast), slast);          // slast_2_sprelast, assumed equal to fh_2_slast
  const Pose lastF_2_slast = poseMul(poseInv(slast), lastF);
  const Pose fhInv = poseInv(fh_2_slast);
  std::vector<Pose> tries;
  tries.push_back(poseMul(fhInv, lastF_2_slast));                       // constant motion
  tries.push_back(poseMul(poseMul(fhInv, fhInv), lastF_2_slast));       // double motion (frame skipped)
  { double lg[6]; poseLogHost(fh_2_slast, lg); for (int i = 0; i < 6; i++) lg[i] *= 0.5; tries.push_back(poseMul(poseInv(poseExp(lg)), lastF_2_slast)); }  // half motion
  tries.push_back(lastF_2_slast);                                       // zero motion
  Pose ident; ident.q.w = 1; ident.q.x = ident.q.y = ident.q.z = 0; ident.t[0] = ident.t[1] = ident.t[2] = 0;
  tries.push_back(ident);                                               // zero motion from the keyframe
  const double d = (double)0.02f;  /* float rotDelta widened by Sophus::Quaterniond */                                              // the reference's rotDelta loop runs exactly once (:376)
  static const int sg[26][3] = {{1,0,0},{0,1,0},{0,0,1},{-1,0,0},{0,-1,0},{0,0,-1},{1,1,0},{0,1,1},{1,0,1},{-1,1,0},{0,-1,1},{-1,0,1},{1,-1,0},{0,1,-1},{1,0,-1},
                                {-1,-1,0},{0,-1,-1},{-1,0,-1},{-1,-1,-1},{-1,-1,1},{-1,1,-1},{-1,1,1},{1,-1,-1},{1,-1,1},{1,1,-1},{1,1,1}};
  const Pose base = poseMul(fhInv, lastF_2_slast);
  for (int k = 0; k < 26; k++) {
    Pose R = ident;
    Quatd q = {1, sg[k][0] * d, sg[k][1] * d, sg[k][2] * d};
    R.q = qnormalize(q);
    tries.push_back(poseMul(base, R));
  }
  const int n = std::min((int)tries.size(), max_out);
  for (int i = 0; i < n; i++) poseTo7(tries[i], out + 7 * i);
  return n;
}

// What trackNewCoarse keeps of one hypothesis.  20 doubles, so that a vector of them IS the buffer the ranks exchange (fp64 sum over the ranks: every record is written
// by its owner, zero elsewhere; x + 0 = x, NaN stays NaN).
struct TryRecord { double pose7[7], aff[2], lastRes[5], flow[3], good, repeated_lvl, first_pass_res; };
static_assert(sizeof(TryRecord) == 20 * sizeof(double), "TryRecord is the exchange format: 20 doubles, no padding");

// Tracks the hypotheses begin, begin + step, ... < end of tries7 as one batch, without abort thresholds, into recs[<index of the try>].  Nothing is written on failure.
static int runTries(dmvio_hip_tracker* t, int new_slot, float new_exposure, const double* tries7, const double aff_last[2], int begin, int step, int end, TryRecord* recs,
                    bool allow_host_lm) {
  const int m = begin < end ? (end - begin + step - 1) / step : 0;
  if (m == 0) return 0;
  std::vector<double> poses(7 * (size_t)m), affs(2 * (size_t)m), lr(5 * (size_t)m), fl(3 * (size_t)m);
  std::vector<int> good(m), slots(m, new_slot);
  std::vector<float> exps(m, new_exposure);
  for (int k = 0; k < m; k++) { memcpy(&poses[7 * (size_t)k], tries7 + 7 * (size_t)(begin + k * step), sizeof(double) * 7); affs[2 * k] = aff_last[0]; affs[2 * k + 1] = aff_last[1]; }
  if (int r = trackBatch(t, m, slots.data(), exps.data(), poses.data(), affs.data(), t->ctx->levels - 1, nullptr, lr.data(), fl.data(), nullptr, nullptr, good.data(), nullptr,
                         allow_host_lm)) return r;
  for (int k = 0; k < m; k++) {
    TryRecord& q = recs[begin + k * step];
    memcpy(q.pose7, &poses[7 * (size_t)k], sizeof(q.pose7)); memcpy(q.aff, &affs[2 * (size_t)k], sizeof(q.aff));
    memcpy(q.lastRes, &lr[5 * (size_t)k], sizeof(q.lastRes)); memcpy(q.flow, &fl[3 * (size_t)k], sizeof(q.flow));
    q.good = good[k]; q.repeated_lvl = t->last.repeat_lvl[k]; q.first_pass_res = t->last.first_pass_res[k];
  }
  return 0;
}

// The sequential rule of the reference's try loop, replayed over records computed without thresholds: the running abort thresholds, the winner so far.
struct TryReplay {
  double achieved[5] = {NAN, NAN, NAN, NAN, NAN};
  bool haveOneGood = false, trackingGood = false;
  int win = -1, used = 0;
};
// Replays the tries [begin, end); true = the loop ends here (the winner so far is under the re-track threshold).  A level residual above 1.5x the running threshold marks
// the try as aborted at that level, exactly as CoarseTracker.cpp:731-732 would have.  Pure host arithmetic.
static bool replayTries(TryReplay& s, const TryRecord* recs, int begin, int end, int L, double reTrackLimit) {
  for (int i = begin; i < end; i++) {
    const TryRecord& q = recs[i];
    s.used++;
    double res[5];
    for (int k = 0; k < 5; k++) res[k] = NAN;
    bool ok = q.good != 0, aborted = false;
    for (int lvl = L - 1; lvl >= 0; lvl--) {
      // a level that ran twice (levelCutoffRepeat) met the abort test after each pass, the first time with the residual the repeat later overwrote
      if (lvl == (int)q.repeated_lvl) {
        const double r1 = q.first_pass_res;
        res[lvl] = r1;
        if (std::isnan(r1) || r1 > 1.5 * s.achieved[lvl]) { aborted = true; break; }
      }
      const double rv = q.lastRes[lvl];
      res[lvl] = rv;
      if (std::isnan(rv) || rv > 1.5 * s.achieved[lvl]) { aborted = true; break; }
    }
    if (aborted) ok = false;
    if (ok) s.trackingGood = true;
    if (ok && std::isfinite((float)res[0]) && !(res[0] >= s.achieved[0])) { s.haveOneGood = true; s.win = i; }
    if (s.haveOneGood)
      for (int k = 0; k < 5; k++)
        if (!std::isfinite((float)s.achieved[k]) || s.achieved[k] > res[k]) s.achieved[k] = res[k];
    if (s.haveOneGood && s.achieved[0] < reTrackLimit) return true;
  }
  return false;
}

// The try loop of FullSystem::trackNewCoarse (FullSystem.cpp:419-489).  The reference runs the hypotheses one after the other, feeding
// the best residuals so far (achievedRes) to the next try as abort thresholds.  Here try 0 runs alone (the usual winner); only if it
// misses the re-track threshold the remaining tries run as ONE batch without thresholds, and the sequential rule is replayed on
// their per-level residuals (a level repeated after levelCutoffRepeat is tested with the residual of each of its two passes) — per-level
// results do not depend on the thresholds, so the outcome is identical.
int dmvio_hip_tracker_track_new_coarse(dmvio_hip_tracker* t, int new_slot, float new_exposure, int n_tries, const double* tries7, const double aff_last[2],
                                       double lastCoarseRMSE_io[5], double reTrackThreshold, double pose7_out[7], double aff_out[2], double flow_out[3],
                                       int* winner, int* tries_used, int* tracking_good) {
  if (!t || !tries7 || !aff_last || !lastCoarseRMSE_io || !pose7_out || !aff_out) return failmsg("track_new_coarse: null argument");
  if (n_tries < 1) return failmsg("track_new_coarse: no hypotheses");
  const int L = t->ctx->levels;
  const double reTrackLimit = lastCoarseRMSE_io[0] * reTrackThreshold;
  // one record per try, and behind them one slot that counts the ranks whose share FAILED locally (see below); records 1 .. n_tries-1 and that slot are the exchange buffer
  std::vector<TryRecord> recs((size_t)n_tries + 1);
  TryReplay s;
  if (int r = runTries(t, new_slot, new_exposure, tries7, aff_last, 0, 1, 1, recs.data(), true)) return r;
  if (!replayTries(s, recs.data(), 0, 1, L, reTrackLimit) && n_tries > 1) {
    const bool split = t->xworld >= 1 && (bool)t->xchg;   // xworld == 1 only through the test hook of dmv_tracker_set_exchange: the whole exchange path on one device
    if (!split) {
      if (int r = runTries(t, new_slot, new_exposure, tries7, aff_last, 1, 1, n_tries, recs.data(), true)) return r;
    } else {
      // the remaining hypotheses over the ranks (try 0 ran on every rank: same inputs, same bits, no exchange when it already ends the loop): rank r takes the tries
      // 1 + r, 1 + r + world, ...; the sum over the ranks hands every rank the complete list, and the sequential rule is replayed identically everywhere.
      // A rank must never leave before the exchange (its peers would wait in the all-reduce for ever): it enters with its error counted in the last slot, and every
      // rank fails together afterwards.  The context's lock is NOT held across the exchange: the RCCL transport works on the context's stream itself.
      double& failed_ranks = recs[n_tries].pose7[0];
      std::string local_err;
      const int local_rc = runTries(t, new_slot, new_exposure, tries7, aff_last, 1 + t->xrank, t->xworld, n_tries, recs.data(), false);
      if (local_rc) { local_err = dmv_err(); failed_ranks = 1.0; }
      if (int r = t->xchg(recs[1].pose7, (size_t)20 * (n_tries - 1) + 1)) return r;
      if (local_rc) return failmsg("track_new_coarse: this rank's share of the hypotheses failed (" + local_err + ")");
      if (failed_ranks != 0.0) return failmsg("track_new_coarse: the share of the hypotheses of " + std::to_string((int)failed_ranks) + " other rank(s) failed");
    }
    replayTries(s, recs.data(), 1, n_tries, L, reTrackLimit);
  }
  const TryRecord* best = s.haveOneGood ? &recs[s.win] : nullptr;
  for (int k = 0; k < 5; k++) lastCoarseRMSE_io[k] = s.achieved[k];
  memcpy(pose7_out, best ? best->pose7 : tries7, sizeof(double) * 7);
  aff_out[0] = best ? best->aff[0] : aff_last[0]; aff_out[1] = best ? best->aff[1] : aff_last[1];
  if (flow_out) for (int k = 0; k < 3; k++) flow_out[k] = best ? best->flow[k] : 0.0;
  if (winner) *winner = s.win;
  if (tries_used) *tries_used = s.used;
  if (tracking_good) *tracking_good = s.trackingGood ? 1 : 0;
  return 0;
}

int dmvio_hip_tracker_debug_split_single_rank(dmvio_hip_tracker* t, int on) {
  if (!t) return failmsg("null tracker");
  t->debug_split1 = on != 0;
  return 0;
}
#ifdef DMV_LM_TICKS
int dmvio_hip_debug_lm_ticks(double out8[8], int reset) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_lm_ticks), sizeof(double) * 8));
  if (reset) { double z[8] = {0}; HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_lm_ticks), z, sizeof(z))); }
  return 0;
}
int dmvio_hip_debug_lm_epilogue(double out4[4], int reset) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_lm_epi), sizeof(double) * 4));
  if (reset) { double z[4] = {0}; HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_lm_epi), z, sizeof(z))); }
  return 0;
}
#endif
int dmvio_hip_tracker_last_ticks(dmvio_hip_tracker* t, long long* ticks_step, long long* ticks_eval) {
  if (!t) return failmsg("null tracker");
  if (ticks_step) *ticks_step = t->last.ticks_step;
  if (ticks_eval) *ticks_eval = t->last.ticks_eval;
  return 0;
}

// Diagnostics: the evaluation loop's division (refined reciprocal shared by the quotients of one denominator) next to the compiler's
// IEEE division, for n operand pairs — lets a test pin the claim that both give the same bits in the operand range of the path.
int dmvio_hip_selftest_divide(dmvio_hip_ctx* c, int n, const float* a, const float* b, float* q_shared, float* q_ieee) {
  if (!c || n <= 0 || !a || !b || !q_shared || !q_ieee) return failmsg("selftest_divide: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  float* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, sizeof(float) * 4 * (size_t)n));
  HIPCHK(c->bounce.h2d(d, a, sizeof(float) * n, c->stream));
  HIPCHK(c->bounce.h2d(d + n, b, sizeof(float) * n, c->stream));
  hipLaunchKernelGGL(k_selftest_divide, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, d, d + n, d + 2 * (size_t)n, d + 3 * (size_t)n);
  HIPCHK(hipGetLastError());
  HIPCHK(c->bounce.d2h(q_shared, d + 2 * (size_t)n, sizeof(float) * n, c->stream));
  HIPCHK(c->bounce.d2h(q_ieee, d + 3 * (size_t)n, sizeof(float) * n, c->stream));
  HIPCHK(c->bounce.finish(c->stream));
  HIPCHK(hipFree(d));
  return 0;
}

int dmvio_hip_tracker_last_launch(dmvio_hip_tracker* t, int* workgroups_per_problem, int* threads_per_workgroup) {
  if (!t) return failmsg("null tracker");
  if (workgroups_per_problem) *workgroups_per_problem = t->last.cluster;
  if (threads_per_workgroup) *threads_per_workgroup = t->last.threads;
  return 0;
}

int dmvio_hip_tracker_last_work(dmvio_hip_tracker* t, long long* n_evals, long long* n_point_evals) {
  if (!t) return failmsg("null tracker");
  if (n_evals) *n_evals = t->last.evals;
  if (n_point_evals) *n_point_evals = t->last.point_evals;
  return 0;
}

int dmvio_hip_tracker_last_residual_only_work(dmvio_hip_tracker* t, long long* n_evals, long long* n_point_evals) {
  if (!t) return failmsg("null tracker");
  if (n_evals) *n_evals = t->last.res_evals;
  if (n_point_evals) *n_point_evals = t->last.res_point_evals;
  return 0;
}

// ------------------------------------------------------------------ W windows' frames against their own references in one launch
// dmvio_hip_tracker_track_multi: every problem names its window, the kernel (k_track_lm_w) takes that window's reference out of a table in device memory.  The handle owns
// what a call needs besides the trackers it reads — its own pipeline of pinned problem / result records, the cluster exchange buffers, the table with its pinned mirror —
// so single and multi calls on the same trackers may be mixed freely.
// Cluster launches stay within LM_RESIDENT_WORKGROUPS like dmvio_hip_tracker_track_batch's (k_track_lm_w<256, 4, *> keeps four workgroups per CU too).
struct dmvio_hip_track_multi {
  dmvio_hip_ctx* ctx = nullptr;
  int max_windows = 0, max_problems = 0;
  BatchPipeline pipe;
  float* d_cl_part = nullptr;          // LM_RESIDENT_WORKGROUPS x 2 x ACC_PAD partial sums (B x 2 x C x ACC_PAD of a launch, B * C within the bound)
  unsigned int* d_cl_cnt = nullptr;    // arrive counters, one per problem of a cluster launch
  char *h_table = nullptr, *d_table = nullptr;   // packed per call: W TrackerDev records, then ref_of[B]
  int lm_cluster = 0, res_only = 1;
  int last_cluster = 0, last_threads = 0;
  long long last_evals = 0, last_point_evals = 0;
};

dmvio_hip_track_multi* dmvio_hip_track_multi_create(dmvio_hip_ctx* c, int max_windows, int max_problems) {
  if (!c) { failmsg("track_multi_create: null context"); return nullptr; }
  if (max_windows < 1 || max_problems < 1) { failmsg("track_multi_create: max_windows and max_problems must be positive"); return nullptr; }
  HIPCHKP(hipSetDevice(c->device));
  dmvio_hip_track_multi* m = new dmvio_hip_track_multi();
  m->ctx = c; m->max_windows = max_windows; m->max_problems = max_problems;
  const size_t table_bytes = sizeof(TrackerDev) * (size_t)max_windows + sizeof(int) * (size_t)max_problems;
  auto init = [&]() -> int {
    if (int r = m->pipe.reserve(max_problems, c->stream)) return r;
    HIPCHK(hipMalloc((void**)&m->d_cl_part, sizeof(float) * (size_t)LM_RESIDENT_WORKGROUPS * 2 * ACC_PAD));
    HIPCHK(hipMalloc((void**)&m->d_cl_cnt, sizeof(unsigned int) * LM_RESIDENT_WORKGROUPS));
    HIPCHK(hipMalloc((void**)&m->d_table, table_bytes));
    HIPCHK(hipHostMalloc((void**)&m->h_table, table_bytes, hipHostMallocDefault));
    return 0;
  };
  if (init()) { dmvio_hip_track_multi_destroy(m); return nullptr; }
  return m;
}

void dmvio_hip_track_multi_destroy(dmvio_hip_track_multi* m) {
  if (!m) return;
  hipSetDevice(m->ctx->device);
  hipStreamSynchronize(m->ctx->stream);
  m->pipe.release();
  if (m->d_cl_part) hipFree(m->d_cl_part);
  if (m->d_cl_cnt) hipFree(m->d_cl_cnt);
  if (m->d_table) hipFree(m->d_table);
  if (m->h_table) hipHostFree(m->h_table);
  delete m;
}

int dmvio_hip_track_multi_set_launch_shape(dmvio_hip_track_multi* m, int lm_cluster) {
  if (!m) return failmsg("track_multi_set_launch_shape: null handle");
  if (lm_cluster < 0 || lm_cluster > 32) return failmsg("track_multi_set_launch_shape: lm_cluster out of range");
  std::lock_guard<std::mutex> lk(m->ctx->mu);
  m->lm_cluster = lm_cluster;
  return 0;
}
int dmvio_hip_track_multi_set_residual_only_evals(dmvio_hip_track_multi* m, int on) {
  if (!m) return failmsg("track_multi_set_residual_only_evals: null handle");
  std::lock_guard<std::mutex> lk(m->ctx->mu);
  m->res_only = on ? 1 : 0;
  return 0;
}
int dmvio_hip_track_multi_last_launch(dmvio_hip_track_multi* m, int* workgroups_per_problem, int* threads_per_workgroup) {
  if (!m) return failmsg("track_multi_last_launch: null handle");
  std::lock_guard<std::mutex> lk(m->ctx->mu);
  if (workgroups_per_problem) *workgroups_per_problem = m->last_cluster;
  if (threads_per_workgroup) *threads_per_workgroup = m->last_threads;
  return 0;
}
int dmvio_hip_track_multi_last_work(dmvio_hip_track_multi* m, long long* n_evals, long long* n_point_evals) {
  if (!m) return failmsg("track_multi_last_work: null handle");
  std::lock_guard<std::mutex> lk(m->ctx->mu);
  if (n_evals) *n_evals = m->last_evals;
  if (n_point_evals) *n_point_evals = m->last_point_evals;
  return 0;
}

int dmvio_hip_tracker_track_multi(dmvio_hip_track_multi* m, int W, dmvio_hip_tracker* const* trackers, int B, const int* window_of, const int* new_slots,
                                  const float* new_exposures, double* pose7_io, double* aff_io, int coarsestLvl, const double* minRes, double* lastResiduals,
                                  double* lastFlow, double* H, double* b, int* good, int* iterations) {
  // every refusal stands before the first enqueue and before the first write to a caller's array
  if (!m) return failmsg("track_multi: null handle");
  if (!trackers || !window_of || !new_slots || !pose7_io || !aff_io) return failmsg("track_multi: null argument");
  if (W < 1 || W > m->max_windows) return failmsg("track_multi: W outside 1 .. max_windows");
  if (B < 0 || B > m->max_problems) return failmsg("track_multi: B outside 0 .. max_problems");
  dmvio_hip_ctx* c = m->ctx;
  for (int w = 0; w < W; w++) {
    if (!trackers[w]) return failmsg("track_multi: null tracker");
    if (trackers[w]->ctx != c) return failmsg("track_multi: a tracker belongs to another context");
  }
  if (coarsestLvl < 0 || coarsestLvl >= c->levels || coarsestLvl >= 5) return failmsg("track_multi: coarsestLvl out of range");
  std::lock_guard<std::mutex> lk(c->mu);
  for (int w = 0; w < W; w++)
    if (!trackers[w]->haveK || !trackers[w]->haveRef) return failmsg("track_multi: makeK / setCoarseTrackingRef not called on a tracker");
  int pc0 = 0;
  bool any_tiled = false;
  for (int i = 0; i < B; i++) {
    if (window_of[i] < 0 || window_of[i] >= W) return failmsg("track_multi: window_of entry out of range");
    if (new_slots[i] < 0 || new_slots[i] >= c->n_slots) return failmsg("track_multi: frame slot out of range");
    pc0 = std::max(pc0, trackers[window_of[i]]->dev.pc_n[0]);
    any_tiled = any_tiled || c->frames.is_tiled(new_slots[i]);
  }
  if (B == 0) return 0;
  const int C = m->lm_cluster > 0 ? m->lm_cluster : clusterSize(B, pc0);
  if (C > 1 && (long)B * C > LM_RESIDENT_WORKGROUPS)
    return failmsg("track_multi: cluster size too large for the batch (B*C must be <= 1024 resident workgroups)");
  HIPCHK(hipSetDevice(c->device));
  BatchPipeline& pl = m->pipe;
  if (int r = pl.reserve(B, c->stream)) return r;
  int half;
  if (int r = pl.stageInto(&half)) return r;
  // the table as the trackers stand now (a set_ref since the last call is seen), then which record each problem reads
  TrackerDev* h_refs = reinterpret_cast<TrackerDev*>(m->h_table);
  int* h_ref_of = reinterpret_cast<int*>(m->h_table + sizeof(TrackerDev) * (size_t)W);
  for (int w = 0; w < W; w++) h_refs[w] = trackers[w]->dev;
  memcpy(h_ref_of, window_of, sizeof(int) * (size_t)B);
  LMProblemIn* in = pl.in(half);
  packProblems(in, B, new_slots, new_exposures, pose7_io, aff_io, minRes);
  pl.stageDone(half, B, coarsestLvl);
  HIPCHK(hipMemcpyAsync(m->d_table, m->h_table, sizeof(TrackerDev) * (size_t)W + sizeof(int) * (size_t)B, hipMemcpyHostToDevice, c->stream));
  ClusterArgs cl = clusterArgs(C, pl.d_discard, m->res_only);
  if (C > 1) {
    HIPCHK(hipMemsetAsync(m->d_cl_cnt, 0, sizeof(unsigned int) * B, c->stream));
    cl.part = m->d_cl_part; cl.cnt = m->d_cl_cnt;
  }
  const TrackerDev* d_refs = reinterpret_cast<const TrackerDev*>(m->d_table);
  const int* d_ref_of = reinterpret_cast<const int*>(m->d_table + sizeof(TrackerDev) * (size_t)W);
  LMProblemOut* pout = pl.out(half);
  pl.unlaunched = false;
  auto lm = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(B * C), dim3(256), 0, c->stream, d_refs, d_ref_of, c->frames.built_on_stream(), (const LMProblemIn*)in, pout, coarsestLvl, cl); };
  if (any_tiled) lm(k_track_lm_w<256, 4, true>); else lm(k_track_lm_w<256, 4, false>);
  HIPCHK(hipGetLastError());
  m->last_cluster = C; m->last_threads = 256;
  if (int r = pl.launched(c->stream)) return r;
  int nB;
  if (int r = pl.take(&half, &nB)) return r;
  const LmWork work = unpackResults(pl.out(half), B, pose7_io, aff_io, lastResiduals, lastFlow, H, b, good, iterations);
  m->last_evals = work.evals; m->last_point_evals = work.point_evals;
  return 0;
}

}  // extern "C"
