// The window optimiser's handle (include/dmvio_hip.h, "sliding-window BA"): struct dmvio_hip_ba, its lock and ready checks, and the transitions of the caches that the
// host-driven loop (ba_loop_host.hpp: GnIteration) and the device-resident loop (ba_batch_host.hpp) leave to each other.  A declaration file of capi_ba.hip's translation
// unit: included there behind ba_kernels.hpp / ba_host.hpp (the types the handle holds) and rccl_api.h, in front of the unit's other host pieces — ba_shard_host.hpp (the
// exchanges of a sharded window), ba_loop_host.hpp (the host loop), ba_graph_host.hpp (the graph build) and ba_batch_host.hpp.
#pragma once
#include <chrono>
// optional host-side time split of the GN iteration (DMVIO_HIP_BA_TIMING=1 prints it when the handle is destroyed)
struct BATimes { double t[8] = {0, 0, 0, 0, 0, 0, 0, 0}; long n = 0; };
static inline double nowUs() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct dmvio_hip_ba {
  // The mapping side owns a HIP stream and a lock of its own: the tracking thread (context stream, context lock) and the mapping
  // thread (this stream, this lock) overlap on the device like coarseTracker / mapping do in the reference (FullSystem.cpp:980-985).
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::recursive_mutex mu;   // every entry point that takes the handle holds it from its first line (entry points may call each other: recursive)
  dmvio_hip_ctx* ctx = nullptr;
  DmvBounce bounce;   // caller-owned arrays (and this file's short-lived host vectors) cross PCIe through the library's pinned memory (internal.h), on `stream`, under `mu`
  BAHost H;
  BAWindow W{};
  BAPoints P{};
  BARes Rs{};
  // host copies of the graph
  std::vector<int> h_host, h_point, h_target, h_res_begin;
  std::vector<int> h_newest;   // residuals that target the newest keyframe (inputs of setNewFrameEnergyTH), ascending
  // device storage.  The window is rebuilt for every keyframe (dmvio_hip_ba_set_graph): its ~75 device arrays are carved out of a few large chunks that stay with the
  // handle and are cleared with one memset each — not allocated, cleared and freed one by one (that cost milliseconds per keyframe, more than optimize(6) itself)
  std::vector<void*> allocs;
  struct Arena { std::vector<std::pair<char*, size_t>> chunks; std::vector<size_t> used; size_t cur = 0, off = 0; bool on = false; } arena;   // used[k]: bytes of chunk k handed out since it was last cleared
  size_t cap_spart = 0, cap_idepth_backup = 0;   // capacities of the grow-only pinned host buffers
  BAPrecalc* d_pre = nullptr;        // [F*F]: the precalc table the kernels read (a rejected step relinearises from the backed-up pair terms it gets as a kernel argument)
  double *d_adHost = nullptr, *d_adTarget = nullptr;
  int *d_top_begin = nullptr, *d_top_members = nullptr, *d_scd_begin = nullptr, *d_scd_members = nullptr;
  float *d_accTop = nullptr, *d_accD = nullptr, *d_accE = nullptr, *d_accC = nullptr;
  int *d_numTop = nullptr, *d_numD = nullptr;
  StitchBufs SB{};
  double *h_sys = nullptr;     // [H_A | b_A | H_sc | b_sc | resInA]: pinned host memory, written by k_ba_stitch_gather
  float *d_spart = nullptr, *h_spart = nullptr;  // point-step partial sums
  // pinned staging for the per-linearisation precalc upload (no pageable copy, no sync before the kernel that consumes it); two, used in turn: an upload may still be
  // in flight behind a linearisation the host did not wait for
  BAPrecalc* h_pre[2] = {nullptr, nullptr};
  int pre_toggle = 0;
  float* d_fullJ = nullptr;
  // device-side decisions (ba_kernels.hpp, BACtl): control block, host-coherent result block, device copies of what the decisions read
  BACtl* d_ctl = nullptr;
  BAHostRes* h_res = nullptr;
  bool th_pending = false;            // the newest keyframe's threshold of the last accept-test pass is stored a few microseconds behind its decision (BAHostRes::th_ticket)
  unsigned int th_pending_ticket = 0;
  float *d_frameTH = nullptr, *h_frameTH = nullptr;   // FrameHessian::frameEnergyTH of every keyframe (the newest one is updated on the device)
  bool th_dirty = true;        // the host changed a threshold: upload before the next linearisation
  double* d_epart = nullptr;
  int* d_newestSlot = nullptr;   // per residual: its position among the residuals that target the newest keyframe, or -1
  float* d_newestE = nullptr;    // their state_NewEnergyWithOutlier, contiguous
  ResubArgs x_none{};            // placeholder argument of linearisations without the fused back-substitution
  BAPreDyn dyn_cur;              // step-dependent precalc members of the CURRENT state (kernel argument of the GN loop's linearisations)
  bool pre_static_valid = false; // the device table holds the evaluation-point members (R0, t0, b0) of the current window
  float* d_newEnergyWO = nullptr;
  unsigned int ticket = 0, acc_ticket = 0;
  float th_cap = -1.0f;        // IMUIntegration::newFrameEnergyTH cap (<= 0: none)
  // a rejected step whose relinearisation the host has not waited for (the loop inside dmvio_hip_ba_optimize): its energy / threshold are picked up at the next wait
  bool pending_reject = false;
  unsigned int pending_ticket = 0;
  int pending_trace = -1;
  bool sys_ready = false;      // h_sys holds the stitched system of the CURRENT state (left behind by the previous GN iteration's chain)
  int n_lin_blocks = 0, n_pt_blocks = 0, n_pt8_blocks = 0, n_epart = 0;   // n_pt8: kernels with eight lanes per point
  bool keep_fullJ = false;   // the 74-float RawResidualJacobian is only materialised on request (dmvio_hip_ba_keep_jacobians) and for marginalisation
  // partial accumulators per bucket: k > 1 = the structure of the reference's multi-threaded accumulation (per-worker fp32 accumulators summed
  // in double, AccumulatedTopHessian.h:91-139) with a FIXED assignment of members to partials; 1 = the reference's single-threaded order, bit for bit
  int nsTop = 4, nsD = 4, nsC = 16;
  bool graph_ready = false;
  // energies of the last optimize
  double trace[64][4];
  int iterations_done = 0;
  double final_energy = 0;
  BATimes tm;
  bool timing = false;
  double tm_graph[6] = {0, 0, 0, 0, 0, 0}; long tm_graph_n = 0;   // dmvio_hip_ba_set_graph: drain + arena memset, host lists, allocation, uploads, pinned buffers + slot table, adjoints + final wait
  // point marginalisation scratch (dmvio_hip_ba_marginalize_points)
  unsigned char *d_cand = nullptr, *d_decision = nullptr, *d_margActive = nullptr;
  float *d_mHdiF = nullptr, *d_mbdSumF = nullptr, *d_mHcd = nullptr, *d_margRec = nullptr, *d_adHTdelta = nullptr;
  long long* d_accTicks = nullptr;   // per-block stamps of k_ba_accumulate (timing mode only)
  int accTicksBlocks = 0;
  // flat arrays of dmvio_hip_ba_set_graph_from (kept between keyframes: no allocation in the steady state)
  struct GraphScratch { std::vector<int> host, res_point, res_target; std::vector<float> u, v, idepth, color, weights, linJ, linRtz; std::vector<unsigned char> prior, lin; } gscratch;
  // ---- points sharded over ranks (dmvio_hip_ba_set_comm): every rank holds all keyframes and ITS points; the stitched system is summed by
  // an all-reduce in HBM on this handle's stream, the accept / threshold decisions are taken over the all-gathered per-rank records
  int rank = 0, world = 0;           // world == 0: no communicator
  ncclComm_t nccl = nullptr;         // RCCL communicator (not owned)
  dmvio_hip_comm_callbacks comm_cb{};   // host-staged transport (MPI, gloo, ...) when nccl == NULL
  double* d_sys = nullptr;           // [H_A | b_A | H_sc | b_sc | resInA] of this rank's points, all-reduced in place
  float *d_xchg_local = nullptr, *d_xchg_all = nullptr;
  int xchg_width = 0;                // floats per rank record: BA_XCHG_HEADER + the largest per-rank count of residuals that target the newest keyframe
  std::vector<double> h_stage;       // callback transport only
  // ---- the reference's DEFAULT solver branch (setting_useGTSAMIntegration, dmvio_hip_ba_optimize_vio): hooks of the running call, the dynamic weight,
  // PointHessian::idepth_backup mirrored into host-coherent memory by the per-point sums (the |idepth_backup| sum of doStepFromBackup's canbreak test)
  const dmvio_hip_ba_callbacks* vio = nullptr;
  const dmvio_hip_ba_vio_options* vio_opt = nullptr;
  double dynW = 1.0;
  int resInA_solve = 0;              // ef->resInA as the reference holds it: set by the accumulation of the last solveSystemF
  float* h_idepth_backup = nullptr;
  std::vector<dmvio_hip_ba_frame_view> vio_frames;
  hipEvent_t* prof = nullptr;        // dmvio_hip_ba_profile_chain: six events recorded between the launches of linearise -> per-point sums -> accumulate -> stitch -> gather
  // dmvio_hip_ba_set_device_loop: dmvio_hip_ba_optimize runs the device-resident loop (a batch of one window) instead of the host-driven one
  bool device_loop = false;
  struct dmvio_hip_ba_batch* own_batch = nullptr;
  // dmvio_hip_ba_comm_timing: HIP events around the collectives of the sharded iteration (RCCL transport), kind 0 = all-reduce of the packed system, 1 = all-gather of the
  // decision records; up to COMM_EVS of each are kept and summed when asked for
  enum { COMM_EVS = 64 };
  bool comm_timing = false;
  hipEvent_t comm_ev[2][COMM_EVS][2] = {};
  int comm_n[2] = {0, 0};
  long comm_total[2] = {0, 0};
  // ---- residuals kept linearised outside a marginalisation (dmvio_hip_ba_fix_linearization; ba_kernels.hpp "residuals kept linearised"): flags, res_toZeroF, the record
  // addPoint<1> consumes, the activity views of the three accumulation passes, the per-point LF sums; host copies of what calcLEnergyPt reads
  int n_lin = 0;
  long long n_lin_global = 0;   // sharded window: the ranks' n_lin summed (dmvio_hip_ba_fix_linearization is collective there) — every rank takes the three-pass accumulation or none
  double* d_red1 = nullptr;     // one double for small all-reduces (the linearised energy of a sharded window)
  unsigned char *d_lin = nullptr, *d_linMask = nullptr, *d_linActive = nullptr, *d_topActive = nullptr;
  float *d_rtz = nullptr, *d_linRec = nullptr, *d_lHdd = nullptr, *d_lbd = nullptr, *d_lHcd = nullptr, *d_HcdAF = nullptr, *d_linE = nullptr;
  std::vector<unsigned char> h_lin, h_linAct;
  std::vector<float> h_linJ, h_rtz;
  bool fullJ_applied = false;   // d_fullJ holds the Jacobians of the APPLIED linearisation (the last linearisation was followed by its applyRes)
  bool adj_dirty = false;   // the host's adjoint tables (H.adHost / adTarget) are newer than the device copy: uploaded by the next consumer (accumulateViews, a batch call)

  // ---- what the accumulation launches of the host loop and of the batched drivers share: the kernel's view of the buckets and its grid (one workgroup per calibration
  // partial and per top partial, four Schur partials per workgroup)
  AccumArgs accumArgs() const {
    AccumArgs A{};
    A.F = H.F; A.N = H.N; A.nsTop = nsTop; A.nsD = nsD; A.nsC = nsC;
    A.top_begin = d_top_begin; A.top_members = d_top_members; A.scd_begin = d_scd_begin; A.scd_members = d_scd_members;
    A.accTop = d_accTop; A.accD = d_accD; A.accE = d_accE; A.accC = d_accC; A.numTop = d_numTop; A.numD = d_numD;
    return A;   // (ticks: null)
  }
  int accBlocks() const { const int F2 = H.F * H.F; return nsC + F2 * nsTop + (F2 * H.F * nsD + 3) / 4; }
  // ---- transitions of the caches above.  Outside of these only the state machine itself (GnIteration, settleReject, optimizeImpl) writes sys_ready, pending_reject,
  // pending_trace and pre_static_valid.
  // the state or the graph changed: the stitched system in h_sys is stale
  void stateChanged() { sys_ready = false; }
  // an evaluation point changed (state_zero, a new graph's window): the device table's R0 / t0 / b0 are stale; evalPointUploaded: uploadWindowTables has refreshed them
  void evalPointChanged() { pre_static_valid = false; }
  void evalPointUploaded() { pre_static_valid = true; }
  // dmvio_hip_ba_set_graph: no relinearisation of the old graph is waited for any more, and every device copy of the window's tables and thresholds is the old graph's
  void graphReplaced() { pending_reject = false; pending_trace = -1; pre_static_valid = false; th_dirty = true; sys_ready = false; }
  // A device-resident loop (a batch call) takes this window.  It runs the reference's non-GTSAM branch from a fresh linearisation, so nothing the host loop carried over
  // survives: the hooks of an earlier call, a rejected step not yet settled, the system and sums in hand.  The batched linearisations relinearise and apply every residual
  // without writing d_fullJ (what the buffer holds is no longer the applied state's), the thresholds live in the window's record from here on (the handle's own device
  // copy is stale; the host's values come back with the record), and the pair tables travel with the batch: the handle's own table is not refreshed.
  void deviceLoopTakes() {
    vio = nullptr; vio_opt = nullptr; dynW = 1.0; H.gtsam = false;
    pending_reject = false; pending_trace = -1; stateChanged();
    fullJ_applied = false; th_dirty = true; pre_static_valid = false;
  }
  // ... and gives it back, re-anchored (BAHost::reanchorNewest) and with `dyn` the pair terms of the state it left: the host's adjoint tables are newer than the device
  // copy (nothing in the batch call stitches again: uploaded by the next consumer), no threshold is on its way through BAHostRes::th_ticket (the newest one is read
  // back behind the final linearisation), and h_sys / the per-point sums were never this state's.
  void deviceLoopReturns(const BAPreDyn& dyn) { dyn_cur = dyn; adj_dirty = true; th_pending = false; stateChanged(); }
};
#define BA_LOCK(b) std::lock_guard<std::recursive_mutex> lk_(b->mu)
#define BA_PROF(b, k) do { if ((b)->prof) hipEventRecord((b)->prof[k], (b)->stream); } while (0)
// the handle has a window and a graph, and its device is current; BA_CHECK_LOCKED leaves the loop's caches alone (dmvio_hip_ba_gn_iteration continues from them),
// BA_READY_LOCKED is what every other entry point takes: it may change the state behind the loop's back
#define BA_CHECK_LOCKED(b) do { if (!(b)->graph_ready) return failmsg("ba: set_window + set_graph first"); HIPCHK(hipSetDevice((b)->ctx->device)); } while (0)
#define BA_READY_LOCKED(b) do { BA_CHECK_LOCKED(b); (b)->stateChanged(); } while (0)
// first statement of an entry point: null check, the handle's lock for the whole call (declares a guard in the function's scope), then the state checks
#define BA_READY(b) if (!(b)) return failmsg("ba: null handle"); BA_LOCK(b); BA_READY_LOCKED(b)
