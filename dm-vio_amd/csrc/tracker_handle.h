// the coarse tracker's handle with what it owns on the host (the batch pipeline, the "last launch" record, the ranking tables of setCoarseTrackingRef), shared by capi.hip
// (tracking), capi_ref.hip (the reference template) and capi_comm.hip (the hypothesis exchange).  No kernel header: every type the handle holds is in common.h.
#pragma once
#include <algorithm>
#include <functional>
#include <vector>
#include "common.h"
#include "internal.h"

// The double-buffered batch pipeline of _track_batch_stage / _launch / _fetch_begin / _fetch.  Problems and results live in two halves of pinned host memory used
// alternately (the kernel reads its 120 B per problem and writes its results there directly); an event follows every launch.  The rules, as transitions:
//   * a batch is staged into the half the LAST launch did not use, once the launch before the last one (same half) has completed;
//   * one batch may be staged behind results marked by fetchBegin(), not two (the kernel would overwrite results nobody has read);
//   * the halves cannot grow while such results are pending;
//   * between stageDone() and the launch `unlaunched` holds: a single-frame call must not slip in front of that batch.
struct BatchPipeline {
  dmv::LMProblemIn* h_in = nullptr;
  dmv::LMProblemOut* h_out = nullptr;
  dmv::LMProblemOut* d_discard = nullptr;   // one device entry: where the non-leading workgroups of cluster mode put their result
  hipEvent_t done[2] = {nullptr, nullptr};   // recorded behind each launch: the results of that half are in host memory once it has completed
  int cap = 0;                         // problems per half
  int cur = 0;                         // half of the last launch
  int staged_half = 0, staged_B = 0, staged_coarsest = 0;
  bool unlaunched = false;
  int fetch_half = 0, fetch_B = 0;     // fetchBegin(): the half and size a later take() refers to (0 = none pending)

  dmv::LMProblemIn* in(int half) const { return h_in + (size_t)half * cap; }
  dmv::LMProblemOut* out(int half) const { return h_out + (size_t)half * cap; }

  int reserve(int B, hipStream_t s) {
    if (B <= cap) return 0;
    if (fetch_B > 0) return failmsg("track_batch_stage: a larger batch cannot be staged while the results of the previous one are still to be fetched");
    if (h_in) { HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipFree(d_discard)); HIPCHK(hipHostFree(h_in)); HIPCHK(hipHostFree(h_out)); }
    cap = std::max(B, 64);
    HIPCHK(hipMalloc((void**)&d_discard, sizeof(dmv::LMProblemOut)));
    HIPCHK(hipHostMalloc((void**)&h_in, sizeof(dmv::LMProblemIn) * 2 * cap, hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void**)&h_out, sizeof(dmv::LMProblemOut) * 2 * cap, hipHostMallocDefault));
    return 0;
  }
  // the half the next batch is written into, free to be overwritten when this returns 0
  int stageInto(int* half) {
    *half = cur ^ 1;
    if (fetch_B > 0 && *half == fetch_half)
      return failmsg("track_batch_stage: the results marked by track_batch_fetch_begin have not been fetched yet (one batch may be staged behind them, not two)");
    if (done[*half]) HIPCHK(hipEventSynchronize(done[*half]));
    return 0;
  }
  void stageDone(int half, int B, int coarsest) { staged_half = half; staged_B = B; staged_coarsest = coarsest; unlaunched = true; }
  // a kernel that works on the staged half has been enqueued on `s` (the host may still be unpacking the other half: fetchBegin pipeline)
  int launched(hipStream_t s) {
    cur = staged_half;
    if (!done[cur]) HIPCHK(hipEventCreateWithFlags(&done[cur], hipEventDisableTiming));
    HIPCHK(hipEventRecord(done[cur], s));
    return 0;
  }
  // nothing to enqueue: the next launch goes into the other half and take() waits for this launch's event only
  void fetchBegin() { fetch_B = staged_B; fetch_half = cur; }
  // waits for the results to unpack: those marked by fetchBegin() (they belong to the launch before the last one) or else the last launch's
  int take(int* half, int* B) {
    *B = staged_B; *half = cur;
    if (fetch_B > 0) { *B = fetch_B; fetch_B = 0; *half = fetch_half; }
    if (!done[*half]) return failmsg("track_batch_fetch: nothing launched");
    HIPCHK(hipEventSynchronize(done[*half]));
    return 0;
  }
  void release() {
    hipFree(d_discard);
    for (hipEvent_t e : done) if (e) hipEventDestroy(e);
    if (h_in) hipHostFree(h_in);
    if (h_out) hipHostFree(h_out);
  }
};

// setCoarseTrackingRef: the rank of every point among the points of its level-0 pixel, in index order, by open addressing on the host (k_ref_scatter adds ranks 0 and 1
// together and every further rank in a launch of its own).  Points outside the image get rank 0 (the scatter drops them).  Returns the largest rank, capped at 255.
struct RefRanker {
  std::vector<int> keys, cnt;
  int rank(const int w0, const int h0, const int n, const float* u, const float* v, unsigned char* out) {
    int maxRank = 0;
    size_t cap = 64;
    while (cap < 2 * (size_t)n + 16) cap <<= 1;
    keys.assign(cap, -1); cnt.assign(cap, 0);
    for (int i = 0; i < n; i++) {
      const int ui = (int)(u[i] + 0.5f), vi = (int)(v[i] + 0.5f);
      if (ui < 0 || vi < 0 || ui >= w0 || vi >= h0) { out[i] = 0; continue; }
      const int key = ui + w0 * vi;
      size_t hpos = ((unsigned)key * 2654435761u) & (cap - 1);
      while (keys[hpos] != -1 && keys[hpos] != key) hpos = (hpos + 1) & (cap - 1);
      keys[hpos] = key;
      const int r = cnt[hpos]++;
      out[i] = (unsigned char)std::min(r, 255);
      maxRank = std::max(maxRank, std::min(r, 255));
    }
    return maxRank;
  }
};

// what the "last launch" queries report (dmvio_hip_tracker_last_launch / _last_work / _last_ticks) and what the try loop of trackNewCoarse reads per problem; a fetch and
// a host-LM call assign it whole, a launch sets its shape
struct LastRun {
  int cluster = 0, threads = 0;        // workgroups per problem, threads per workgroup
  long long evals = 0, point_evals = 0, ticks_step = 0, ticks_eval = 0;
  long long res_evals = 0, res_point_evals = 0;   // of evals / point_evals: the residual-only ones (dmvio_hip_tracker_last_residual_only_work)
  int vio_iterations = 0;              // LM iterations of the last host-LM call
  std::vector<int> repeat_lvl;         // per problem: the level that ran twice (or -1) ...
  std::vector<double> first_pass_res;  // ... and its residual after the first pass
};

struct dmvio_hip_tracker {
  dmvio_hip_ctx* ctx = nullptr;
  dmv::TrackerDev dev{};
  bool haveK = false, haveRef = false;
  dmv::RefLevels R{};
  int n_tiles = 0;
  float *d_idp = nullptr, *d_wsp = nullptr, *d_idp2 = nullptr, *d_wsp2 = nullptr, *d_dense = nullptr;
  int *d_tile_count = nullptr, *d_tile_base = nullptr, *d_pc_n = nullptr, *d_seg = nullptr;
  unsigned long long* d_flow_mask = nullptr;
  size_t flow_words = 0;
  float4* d_pc[DMV_MAX_LEVELS] = {};
  float4** d_pc_ptrs = nullptr;
  float* d_pts = nullptr;
  int pts_cap = 0;
  RefRanker ranker;                            // set_ref: host-side ranking of the points that share a pixel
  std::vector<unsigned char> h_rank;
  // set_ref_from_ba (capi_ref.hip): the crowded list ((pixel, residual) pairs, room for every residual of the window: grow-only) — its length and the number of
  // selected residuals stand behind pc_n, d_pc_n[REF_BA_CROWDED] / [REF_BA_SELECTED]; the event the context's stream waits for before it reads a BA handle's arrays, and
  // the one that handle's stream waits for behind the last read
  enum { REF_BA_SELECTED = DMV_MAX_LEVELS, REF_BA_CROWDED = DMV_MAX_LEVELS + 1, PC_N_INTS = DMV_MAX_LEVELS + 2 };
  int2* d_ba_crowded = nullptr;
  int ba_crowded_cap = 0;
  hipEvent_t ev_ba_ready = nullptr, ev_ba_read = nullptr;
  // fused evaluation (k_eval_fused)
  float *d_partials = nullptr, *h_tot = nullptr;
  unsigned int* d_arrive = nullptr;   // arrive counter of k_eval_fused (zero between launches)
  unsigned int eval_ticket = 0;       // ticket of the last fused evaluation; the kernel stores it behind the sums in h_tot
  int eval_blocks_override = 0;
  int max_eval_blocks = 1024;
  // evaluation server (k_eval_server): one launch per tracked frame, requests through a mailbox in host-coherent memory
  unsigned int* d_leave = nullptr;    // the launch (by its first ticket) whose workgroups have been told to leave by an idle time-out
  unsigned int* h_mail = nullptr;     // EVAL_MAIL_DWORDS dwords: [0] request ticket, [1..] EvalP, [last] the ticket again (written before [0])
  float* h_rec = nullptr;             // EVAL_SERVER_MAX_BLOCKS records of EVAL_RECORD_FLOATS floats: every server workgroup stores its partial sums + the ticket into its own
  bool server_on = false;             // a server kernel was launched for server_slot and has not been told to quit
  int server_slot = -1, server_G = 0;
  unsigned int server_session = 0;    // identity of the current serverStart .. serverStop session (mailbox dword EVAL_MAIL_SESSION, kernel argument)
  long long server_idle_ticks = 500000;   // the server leaves after this long without a request (100 MHz ticks: 5 ms); dmvio_hip_tracker_set_server_idle_us
  int use_server = 1;                 // dmvio_hip_tracker_set_eval_server(0): one k_eval_fused launch per evaluation instead
  int single_host_lm = 1;             // dmvio_hip_tracker_set_single_frame_mode(0): a single alignment problem runs the device-resident LM (cluster mode) instead of the host LM + server
  // hypothesis-parallel trackNewCoarse: the tries after the first are split over `xworld` ranks, their per-try records summed over the ranks (every record is written by
  // exactly one rank, the others add zeros) by `xchg`
  std::function<int(double*, size_t)> xchg;
  int xrank = 0, xworld = 0;
  bool debug_split1 = false;          // dmvio_hip_tracker_debug_split_single_rank: a group of ONE rank still takes the split path (tests of the transport on a one-device box)
  // batched device-resident LM
  BatchPipeline pipe;
  LastRun last;
  int batch_kernel = 0;          // dmvio_hip_tracker_set_batch_kernel: 1 = full batches on k_track_lm_pp (control steps beside the evaluations)
  int last_fused_builds = 0;     // dmvio_hip_tracker_last_fused_builds: problems of the last batch launch whose frame's pyramid the tracking kernel built itself (k_track_lm_build)
  int res_only_evals = 1;        // dmvio_hip_tracker_set_residual_only_evals: k_track_lm runs the evaluations whose 9x9 sums nothing reads as residual-only ones
  unsigned int* d_pp_next = nullptr;
  int lm_threads_override = 0, lm_cluster_override = 0;   // dmvio_hip_tracker_set_launch_shape
  float* d_cl_part = nullptr;          // cluster mode: B x 2 x C x ACC_PAD partial sums
  unsigned int* d_cl_cnt = nullptr;    // cluster mode: arrive counters
  size_t cl_part_cap = 0; int cl_cnt_cap = 0;
  int debug_mode = 0, log_cap = 0, log_B = 0;   // dmvio_hip_tracker_debug_record_replay
  dmv::EvalP* d_log = nullptr; int* d_log_n = nullptr; float* d_log_sink = nullptr;
};
