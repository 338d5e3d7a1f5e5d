// libdmvio_hip.so — C ABI implementation (include/dmvio_hip.h), the coarse tracker's reference template: setCoarseTrackingRef of one tracker and of W trackers per call, from
// host arrays or straight out of resident BA windows, and the queries of what it left.  gfx950 only.  The only unit that compiles ref_kernels.hpp and ref_batch_kernels.hpp.
#include <hip/hip_runtime.h>
#include <cstring>
#include <mutex>
#include <vector>
#include <algorithm>

#include "../../include/dmvio_hip.h"
#include "common.h"
#include "ref_kernels.hpp"
#include "ref_batch_kernels.hpp"

using namespace dmv;

#include "tracker_handle.h"

// what ends a setCoarseTrackingRef, single or batched: the template the kernels left (pcn: its points per level) becomes the tracker's reference
static void refPublish(dmvio_hip_tracker* t, const int* pcn, float ref_exposure, double aff_a, double aff_b) {
  for (int l = 0; l < t->R.levels; l++) { t->dev.pc_n[l] = pcn[l]; t->dev.pc[l] = t->d_pc[l]; }
  t->dev.ref_exposure = ref_exposure; t->dev.ref_aff_a = aff_a; t->dev.ref_aff_b = aff_b;
  t->haveRef = true;
}

// the stages behind the scatter of a single call, host arrays or BA window alike: pyramid sums, dilation, ordered compaction (enqueued on the context's stream)
static int refStagesFromPool(dmvio_hip_tracker* t, int ref_slot, hipStream_t s) {
  dmvio_hip_ctx* c = t->ctx;
  const RefLevels& R = t->R;
  if (R.levels > 1) {
    const size_t npool = R.total - R.off[1];
    hipLaunchKernelGGL(k_ref_pool, dim3((unsigned)((npool + 255) / 256)), dim3(256), 0, s, R, t->d_idp, t->d_wsp);
  }
  hipLaunchKernelGGL(k_ref_dilate, dim3((unsigned)((R.total + 255) / 256)), dim3(256), 0, s, R, t->d_idp, t->d_wsp, t->d_idp2, t->d_wsp2);
  HIPCHK(hipMemsetAsync(t->d_flow_mask, 0, sizeof(unsigned long long) * t->flow_words, s));
  hipLaunchKernelGGL(k_ref_count, dim3(t->n_tiles), dim3(256), 0, s, R, t->d_idp2, t->d_wsp2, c->frames.built_and_waited(), ref_slot, t->d_tile_count, t->d_seg);
  hipLaunchKernelGGL(k_ref_scan, dim3(2 * R.levels), dim3(1024), 0, s, R, t->d_tile_count, t->d_tile_base, t->d_pc_n, t->d_seg);
  hipLaunchKernelGGL(k_ref_write, dim3(t->n_tiles), dim3(256), 0, s, R, t->d_idp2, t->d_wsp2, c->frames.built_and_waited(), ref_slot, t->d_tile_base, t->d_seg, t->d_pc_ptrs,
                     t->d_dense, t->d_flow_mask);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" {

int dmvio_hip_tracker_set_ref(dmvio_hip_tracker* t, int ref_slot, float ref_exposure, double aff_a, double aff_b,
                              int n, const float* u, const float* v, const float* idepth, const float* hdiF) {
  if (!t) return failmsg("tracker_set_ref: null tracker");
  dmvio_hip_ctx* c = t->ctx;
  if (ref_slot < 0 || ref_slot >= c->n_slots) return failmsg("tracker_set_ref: slot out of range");
  if (n < 0 || (n > 0 && (!u || !v || !idepth || !hdiF))) return failmsg("tracker_set_ref: bad point arrays");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  if (int r = dmv_ensure_row_major_locked(c, ref_slot)) return r;
  hipStream_t s = c->stream;
  if (n > t->pts_cap) {
    if (t->d_pts) HIPCHK(hipFree(t->d_pts));
    t->pts_cap = std::max(n, 4096);
    HIPCHK(hipMalloc((void**)&t->d_pts, sizeof(float) * 5 * t->pts_cap));   // u, v, idepth, hdiF, [per-pixel rank bytes]
  }
  const RefLevels& R = t->R;
  HIPCHK(hipMemsetAsync(t->d_idp, 0, sizeof(float) * R.w[0] * R.h[0], s));
  HIPCHK(hipMemsetAsync(t->d_wsp, 0, sizeof(float) * R.w[0] * R.h[0], s));
  if (n > 0) {
    HIPCHK(c->bounce.h2d(t->d_pts + 0 * (size_t)t->pts_cap, u, sizeof(float) * n, s));      // through the library's pinned memory (internal.h: DmvBounce)
    HIPCHK(c->bounce.h2d(t->d_pts + 1 * (size_t)t->pts_cap, v, sizeof(float) * n, s));
    HIPCHK(c->bounce.h2d(t->d_pts + 2 * (size_t)t->pts_cap, idepth, sizeof(float) * n, s));
    HIPCHK(c->bounce.h2d(t->d_pts + 3 * (size_t)t->pts_cap, hdiF, sizeof(float) * n, s));
    // rank of every point among the points of its pixel (index order): pixels with more than two points are scattered rank by rank (k_ref_scatter)
    t->h_rank.resize(n);
    const int maxRank = t->ranker.rank(R.w[0], R.h[0], n, u, v, t->h_rank.data());
    const unsigned char* d_rank = nullptr;
    if (maxRank >= 2) {
      HIPCHK(c->bounce.h2d(t->d_pts + 4 * (size_t)t->pts_cap, t->h_rank.data(), (size_t)n, s));
      d_rank = (const unsigned char*)(t->d_pts + 4 * (size_t)t->pts_cap);
    }
    for (int r = 1; r <= std::max(maxRank, 1); r++)
      hipLaunchKernelGGL(k_ref_scatter, dim3((n + 255) / 256), dim3(256), 0, s, n, t->d_pts, t->d_pts + t->pts_cap, t->d_pts + 2 * (size_t)t->pts_cap,
                         t->d_pts + 3 * (size_t)t->pts_cap, t->d_idp, t->d_wsp, R.w[0], R.h[0], d_rank, r == 1 ? 0 : r, r);
  }
  if (int r = refStagesFromPool(t, ref_slot, s)) return r;
  int pcn[DMV_MAX_LEVELS] = {};
  HIPCHK(c->bounce.d2h(pcn, t->d_pc_n, sizeof(int) * R.levels, s));
  HIPCHK(c->bounce.finish(s));
  refPublish(t, pcn, ref_exposure, aff_a, aff_b);
  return 0;
}

int dmvio_hip_tracker_pc_n(dmvio_hip_tracker* t, int lvl) {
  if (!t || lvl < 0 || lvl >= t->ctx->levels) return failmsg("tracker_pc_n: bad argument");
  return t->dev.pc_n[lvl];
}

int dmvio_hip_tracker_get_pc(dmvio_hip_tracker* t, int lvl, float* u, float* v, float* idepth, float* color) {
  if (!t || lvl < 0 || lvl >= t->ctx->levels) return failmsg("tracker_get_pc: bad argument");
  dmvio_hip_ctx* c = t->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  const int n = t->dev.pc_n[lvl];
  std::vector<float4> tmp(n);
  HIPCHK(c->bounce.d2h(tmp.data(), t->d_pc[lvl], sizeof(float4) * n, c->stream));
  HIPCHK(c->bounce.finish(c->stream));
  // the device keeps the template in tile order; hand it out in the reference's row-major order (y, then x)
  std::sort(tmp.begin(), tmp.end(), [](const float4& a, const float4& b) { return a.y < b.y || (a.y == b.y && a.x < b.x); });
  for (int i = 0; i < n; i++) { u[i] = tmp[i].x; v[i] = tmp[i].y; idepth[i] = tmp[i].z; color[i] = tmp[i].w; }
  return 0;
}

// The dense maps CoarseTracker keeps next to the template: idepth[lvl] and weightSums[lvl] as makeCoarseDepthL0 leaves them (CoarseTracker.cpp:249-293; read by
// debugPlotIDepthMap / debugPlotIDepthMapFloat, :772-880, when output wrappers exist).  Debug path: the dilated planes come back from the device and the normalisation loop is
// replayed on the host; whether a pixel with weight became a template point (finite reference colour, idepth > 0) is taken from the template itself.
int dmvio_hip_tracker_get_idepth_map(dmvio_hip_tracker* t, int lvl, float* idepth_out, float* weightSums_out) {
  if (!t || lvl < 0 || lvl >= t->ctx->levels || !idepth_out) return failmsg("tracker_get_idepth_map: bad argument");
  if (!t->haveRef) return failmsg("tracker_get_idepth_map: setCoarseTrackingRef not called");
  dmvio_hip_ctx* c = t->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  const RefLevels& R = t->R;
  const int wl = R.w[lvl], hl = R.h[lvl], n = t->dev.pc_n[lvl];
  const size_t npx = (size_t)wl * hl;
  std::vector<float> ws(npx);
  std::vector<float4> pc(n);
  HIPCHK(c->bounce.d2h(idepth_out, t->d_idp2 + R.off[lvl], sizeof(float) * npx, c->stream));
  HIPCHK(c->bounce.d2h(ws.data(), t->d_wsp2 + R.off[lvl], sizeof(float) * npx, c->stream));
  if (n) HIPCHK(c->bounce.d2h(pc.data(), t->d_pc[lvl], sizeof(float4) * n, c->stream));
  HIPCHK(c->bounce.finish(c->stream));
  std::vector<unsigned char> kept(npx, 0);
  for (int i = 0; i < n; i++) kept[(size_t)pc[i].x + (size_t)pc[i].y * wl] = 1;
  for (int y = 2; y < hl - 2; y++)
    for (int x = 2; x < wl - 2; x++) {
      const size_t i = (size_t)x + (size_t)y * wl;
      if (ws[i] > 0) {
        idepth_out[i] /= ws[i];
        if (!kept[i]) { idepth_out[i] = -1; continue; }   // the reference's "just skip if something is wrong": weightSums keeps its value
      } else
        idepth_out[i] = -1;
      ws[i] = 1;
    }
  if (weightSums_out) memcpy(weightSums_out, ws.data(), sizeof(float) * npx);
  return 0;
}
// Order in which setCoarseTrackingRef stores the template points of every level: 0 (default) = 8x8-pixel tiles, Z-ordered inside 16x16 blocks; 1 = the reference's
// row-major order (CoarseTracker.cpp:249-293).  Takes effect with the next dmvio_hip_tracker_set_ref.  The sums of an evaluation are formed per 64-point group and then in
// group order, so the two orders group the fp32 additions differently (results agree to rounding, like cluster sizes do); profiles/r05_tracker_floor.md has the measurement.
int dmvio_hip_tracker_set_template_order(dmvio_hip_tracker* t, int row_major) {
  if (!t) return failmsg("null tracker");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  t->R.order = row_major ? 1 : 0;
  return 0;
}

// ------------------------------------------------------------------ W trackers' reference templates in one pass
// dmvio_hip_tracker_set_ref_batch: setCoarseTrackingRef + makeCoarseDepthL0 (CoarseTracker.cpp:524-538, 138-295) of W trackers of one context.  The handle owns what a call
// needs besides the trackers' own buffers: a slab in pinned memory with its device copy (W RefWin records, the four point arrays of every window, their rank bytes: one
// upload), the [W][levels] pc_n table with its pinned mirror (one download) and the ranking tables.  Every kernel runs over all W windows (ref_batch_kernels.hpp); the
// trackers' scratch for the single call (d_pts) is not touched, so single and batched calls on one tracker may be mixed freely.
struct dmvio_hip_set_ref_batch {
  dmvio_hip_ctx* ctx = nullptr;
  int max_windows = 0, max_points = 0;
  DmvSlab slab;   // records, then floats, then bytes, or the records of a from-BA call (dmvRefSlabBytes, batch_slab.hpp); sized at creation
  DmvSlab pcn;    // ints [max_windows][DMV_MAX_LEVELS + 1]; a call uses [W][levels], a from-BA call W selected counts behind them
  RefRanker ranker;
  DmvWork work;   // of the last call
};
static const char* const REF_HEAD_TEXT[3] = {": null handle", ": W outside 0 .. max_windows", ": null window array"};

// a tracker's buffers as the W-window kernels find them; the points of the window (none here) are the caller's part
static void refWinRecord(RefWin& V, dmvio_hip_tracker* t, int* pc_n_row, int ref_slot) {
  V.idp = t->d_idp; V.wsp = t->d_wsp; V.idp2 = t->d_idp2; V.wsp2 = t->d_wsp2; V.dense = t->d_dense;
  V.tile_count = t->d_tile_count; V.tile_base = t->d_tile_base; V.seg = t->d_seg; V.pc_n = t->d_pc_n;
  V.pc = t->d_pc_ptrs; V.flow_mask = t->d_flow_mask;
  V.pc_n_row = pc_n_row;
  V.pts_off = 0; V.rank_off = 0;
  V.ref_slot = ref_slot; V.n = 0; V.order = t->R.order; V.max_rank = 0;
}

dmvio_hip_set_ref_batch* dmvio_hip_set_ref_batch_create(dmvio_hip_ctx* c, int max_windows, int max_points_per_window) {
  if (!c) { failmsg("set_ref_batch_create: null context"); return nullptr; }
  if (max_windows < 1 || max_points_per_window < 1) { failmsg("set_ref_batch_create: max_windows and max_points_per_window must be positive"); return nullptr; }
  HIPCHKP(hipSetDevice(c->device));
  dmvio_hip_set_ref_batch* b = new dmvio_hip_set_ref_batch();
  b->ctx = c; b->max_windows = max_windows; b->max_points = max_points_per_window;
  b->slab.work = b->pcn.work = &b->work;
  if (b->slab.create(dmvRefSlabBytes(sizeof(RefWin), sizeof(RefBaWin), max_windows, max_points_per_window)) ||
      b->pcn.create(sizeof(int) * (DMV_MAX_LEVELS + 1) * (size_t)max_windows)) { dmvio_hip_set_ref_batch_destroy(b); return nullptr; }
  return b;
}

void dmvio_hip_set_ref_batch_destroy(dmvio_hip_set_ref_batch* b) {
  if (!b) return;
  hipSetDevice(b->ctx->device);
  hipStreamSynchronize(b->ctx->stream);
  b->slab.release(); b->pcn.release();
  delete b;
}

int dmvio_hip_set_ref_batch_last_work(dmvio_hip_set_ref_batch* b, int* launches, int* uploads, int* downloads, int* waits) {
  if (!b) return failmsg("set_ref_batch_last_work: null handle");
  std::lock_guard<std::mutex> lk(b->ctx->mu);
  b->work.report(launches, uploads, downloads, waits);
  return 0;
}

int dmvio_hip_tracker_set_ref_batch(dmvio_hip_set_ref_batch* b, int W, const dmvio_hip_set_ref_window* win) {
  // every refusal stands before the first enqueue and before the first write to a tracker
  if (int r = dmvBatchHead(b, W, b ? b->max_windows : 0, win, "tracker_set_ref_batch", REF_HEAD_TEXT)) return r;
  dmvio_hip_ctx* c = b->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  size_t total = 0;
  int max_n = 0;
  for (int w = 0; w < W; w++) {
    const dmvio_hip_set_ref_window& x = win[w];
    if (!x.trk) return failmsg("tracker_set_ref_batch: null tracker");
    if (x.trk->ctx != c) return failmsg("tracker_set_ref_batch: a tracker belongs to another context");
    if (x.ref_slot < 0 || x.ref_slot >= c->n_slots) return failmsg("tracker_set_ref_batch: slot out of range");
    if (x.n < 0 || x.n > b->max_points) return failmsg("tracker_set_ref_batch: n outside 0 .. max_points_per_window");
    if (x.n > 0 && (!x.u || !x.v || !x.idepth || !x.hdiF)) return failmsg("tracker_set_ref_batch: null point array");
    total += (size_t)x.n;
    max_n = std::max(max_n, x.n);
  }
  if (dmvFirstRepeated(win, W, &dmvio_hip_set_ref_window::trk) >= 0)
    return failmsg("tracker_set_ref_batch: the same tracker is named twice (two windows would write one set of buffers)");
  b->work.clear();
  if (W == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  // reference slots whose level 0 is stored in 8x4 tiles go back to row-major first, as in the single call (their launches are not part of last_work's figures)
  for (int w = 0; w < W; w++) if (int r = dmv_ensure_row_major_locked(c, win[w].ref_slot)) return r;
  hipStream_t s = c->stream;
  RefLevels R = win[0].trk->R;   // the geometry is the context's, the same for every tracker; the storage order is the tracker's and travels in its record
  R.order = 0;
  const int n_tiles = win[0].trk->n_tiles, flow_words = (int)win[0].trk->flow_words;
  const int n0 = R.w[0] * R.h[0];
  // the slab: caller arrays are copied into the handle's pinned memory (internal.h: DmvBounce has the reason) and go up in one copy
  if (int r = b->slab.begin(s)) return r;
  DmvCursor L;
  RefWin* h_wins = b->slab.host<RefWin>(dmvRecords(L, sizeof(RefWin), W));
  size_t pts = dmvRefPoints(L, total) / sizeof(float), ranks = dmvRefRanks(L, total);
  int* const d_pcn = b->pcn.dev<int>(0); const int* const h_pcn = b->pcn.host<int>(0);
  int max_rank = 0;
  for (int w = 0; w < W; w++) {
    const dmvio_hip_set_ref_window& x = win[w];
    dmvio_hip_tracker* t = x.trk;
    RefWin& V = h_wins[w];
    refWinRecord(V, t, d_pcn + (size_t)w * R.levels, x.ref_slot);
    V.pts_off = pts; V.rank_off = ranks; V.n = x.n;
    if (x.n > 0) {
      float* hp = b->slab.host<float>(0) + pts;
      memcpy(hp, x.u, sizeof(float) * x.n); memcpy(hp + x.n, x.v, sizeof(float) * x.n);
      memcpy(hp + 2 * (size_t)x.n, x.idepth, sizeof(float) * x.n); memcpy(hp + 3 * (size_t)x.n, x.hdiF, sizeof(float) * x.n);
      V.max_rank = b->ranker.rank(R.w[0], R.h[0], x.n, x.u, x.v, b->slab.host<unsigned char>(ranks));
    }
    max_rank = std::max(max_rank, V.max_rank);
    pts += 4 * (size_t)x.n; ranks += (size_t)x.n;
  }
  if (int r = b->slab.upload(s, L.bytes())) return r;
  const RefWin* d_wins = b->slab.dev<const RefWin>(0);
  const float* d_slab = b->slab.dev<const float>(0);
  int& launches = b->work.launches;
  const unsigned gw = (unsigned)W;
  hipLaunchKernelGGL(k_ref_clear_w, dim3((unsigned)(((n0 + 3) / 4 + 255) / 256), gw), dim3(256), 0, s, d_wins, n0, flow_words); launches++;
  // ranks 0 and 1 together, then every further rank of the batch behind them: a window whose own largest rank is below the launch's leaves at once
  const unsigned gs = (unsigned)std::max(1, (max_n + 255) / 256);
  for (int r = 1; r <= std::max(max_rank, 1); r++) {
    hipLaunchKernelGGL(k_ref_scatter_w, dim3(gs, gw), dim3(256), 0, s, d_wins, d_slab, R.w[0], R.h[0], r == 1 ? 0 : r, r); launches++;
  }
  if (R.levels > 1) {
    const size_t npool = R.total - R.off[1];
    hipLaunchKernelGGL(k_ref_pool_w, dim3((unsigned)((npool + 255) / 256), gw), dim3(256), 0, s, d_wins, R); launches++;
  }
  hipLaunchKernelGGL(k_ref_dilate_w, dim3((unsigned)((R.total + 255) / 256), gw), dim3(256), 0, s, d_wins, R); launches++;
  hipLaunchKernelGGL(k_ref_count_w, dim3(n_tiles, gw), dim3(256), 0, s, d_wins, R, c->frames.built_and_waited()); launches++;
  hipLaunchKernelGGL(k_ref_scan_w, dim3(2 * R.levels, gw), dim3(1024), 0, s, d_wins, R); launches++;
  hipLaunchKernelGGL(k_ref_write_w, dim3(n_tiles, gw), dim3(256), 0, s, d_wins, R, c->frames.built_and_waited()); launches++;
  HIPCHK(hipGetLastError());
  if (int r = b->pcn.download(s, 0, sizeof(int) * (size_t)W * R.levels)) return r;
  if (int r = b->slab.wait(s)) return r;
  for (int w = 0; w < W; w++) refPublish(win[w].trk, h_pcn + (size_t)w * R.levels, win[w].ref_exposure, win[w].ref_aff_a, win[w].ref_aff_b);
  return 0;
}

}  // extern "C"

// ------------------------------------------------------------------ the template straight out of resident BA windows
// dmvio_hip_tracker_set_ref_from_ba / _from_ba_batch: what setCoarseTrackingRef reads per point (CoarseTracker.cpp:138-161: centerProjectedTo of the residual to the newest
// keyframe, efPoint->HdiF) is on the device when dmvio_hip_ba_optimize returns; the scatter reads it there (ref_kernels.hpp: refBaCountBody / ScatterBody / CrowdedBody) and
// every later stage is the host-array call's.
// Locks: the BA handles of the call first, in address order (as the BA batches take them), then the context's.  BA code never takes the context's lock, so the order
// cannot deadlock with a mapping thread that holds a BA handle.
// Streams: the arrays are written on the BA handle's stream, the template is built on the context's.  No host wait orders them: an event recorded on the handle's stream
// is waited for by the context's stream in front of the first kernel that reads the handle, and an event recorded on the context's stream behind the last such kernel
// (the crowded pass) is waited for by the handle's stream — a dmvio_hip_ba_set_graph that follows cannot overwrite what the scatter still reads.
struct RefBaLocks {
  std::vector<dmvio_hip_ba*> held;
  void lock(std::vector<dmvio_hip_ba*> v) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    for (dmvio_hip_ba* b : v) { dmv_ba_lock(b); held.push_back(b); }
  }
  ~RefBaLocks() { for (size_t i = held.size(); i-- > 0;) dmv_ba_unlock(held[i]); }
};
// the refusals one window can earn (under the handle's lock and the context's)
static int refBaCheck(const char* who, const dmvio_hip_ctx* c, const dmvio_hip_tracker* t, const DmvBaRefSource& S, int ref_slot) {
  if (t->ctx != c) return failmsg(std::string(who) + ": a tracker belongs to another context");
  if (S.ctx != c) return failmsg(std::string(who) + ": a BA handle belongs to another context");
  // a window of ONE keyframe can hold no residual, so dmvio_hip_ba_set_graph takes no graph for it: it selects nothing and the template ends empty
  if (!S.graph_ready && S.F != 1) return failmsg(std::string(who) + ": a BA handle has no graph (set_window + set_graph first)");
  if (S.sharded) return failmsg(std::string(who) + ": a BA handle is sharded over ranks (it holds a part of the window's points)");
  if (ref_slot < 0 || ref_slot >= c->n_slots) return failmsg(std::string(who) + ": slot out of range");
  return 0;
}
// the tracker's crowded list holds every residual of the window; its two events exist
static int refBaReserve(dmvio_hip_tracker* t, int R) {
  if (R > t->ba_crowded_cap) {
    if (t->d_ba_crowded) HIPCHK(hipFree(t->d_ba_crowded));
    t->d_ba_crowded = nullptr; t->ba_crowded_cap = 0;
    const int cap = std::max(R, 4096);
    HIPCHK(hipMalloc((void**)&t->d_ba_crowded, sizeof(int2) * (size_t)cap));
    t->ba_crowded_cap = cap;
  }
  if (!t->ev_ba_ready) HIPCHK(hipEventCreateWithFlags(&t->ev_ba_ready, hipEventDisableTiming));
  if (!t->ev_ba_read) HIPCHK(hipEventCreateWithFlags(&t->ev_ba_read, hipEventDisableTiming));
  return 0;
}

extern "C" {

int dmvio_hip_tracker_set_ref_from_ba(dmvio_hip_tracker* t, dmvio_hip_ba* ba, int ref_slot, float ref_exposure, double aff_a, double aff_b, int* n_selected) {
  if (!t) return failmsg("tracker_set_ref_from_ba: null tracker");
  if (!ba) return failmsg("tracker_set_ref_from_ba: null BA handle");
  dmvio_hip_ctx* c = t->ctx;
  RefBaLocks bl;
  bl.lock({ba});
  std::lock_guard<std::mutex> lk(c->mu);
  DmvBaRefSource S;
  dmv_ba_ref_source_locked(ba, &S);
  if (int r = refBaCheck("tracker_set_ref_from_ba", c, t, S, ref_slot)) return r;
  HIPCHK(hipSetDevice(c->device));
  if (int r = dmv_ensure_row_major_locked(c, ref_slot)) return r;
  if (int r = refBaReserve(t, S.R)) return r;
  hipStream_t s = c->stream;
  const RefLevels& R = t->R;
  const size_t n0 = (size_t)R.w[0] * R.h[0];
  int* d_cnt = reinterpret_cast<int*>(t->d_idp2);   // selected points per level-0 pixel: k_ref_dilate overwrites the plane later
  HIPCHK(hipMemsetAsync(t->d_idp, 0, sizeof(float) * n0, s));
  HIPCHK(hipMemsetAsync(t->d_wsp, 0, sizeof(float) * n0, s));
  HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(int) * n0, s));
  HIPCHK(hipMemsetAsync(t->d_pc_n + dmvio_hip_tracker::REF_BA_SELECTED, 0, sizeof(int) * 2, s));
  if (S.R > 0) {
    HIPCHK(hipEventRecord(t->ev_ba_ready, S.stream));
    HIPCHK(hipStreamWaitEvent(s, t->ev_ba_ready, 0));
    RefBaSrc src{S.res_point, S.res_target, S.newState, S.active, S.center, S.HdiF, S.R, S.F - 1};
    const dim3 g((unsigned)((S.R + 255) / 256));
    int* d_sel = t->d_pc_n + dmvio_hip_tracker::REF_BA_SELECTED;
    int* d_ncr = t->d_pc_n + dmvio_hip_tracker::REF_BA_CROWDED;
    hipLaunchKernelGGL(k_ref_ba_count, g, dim3(256), 0, s, src, R.w[0], R.h[0], d_cnt, d_sel);
    hipLaunchKernelGGL(k_ref_ba_scatter, g, dim3(256), 0, s, src, t->d_idp, t->d_wsp, R.w[0], R.h[0], (const int*)d_cnt, d_ncr, t->d_ba_crowded, t->ba_crowded_cap);
    hipLaunchKernelGGL(k_ref_ba_crowded, g, dim3(256), 0, s, src, t->d_idp, t->d_wsp, (const int*)d_ncr, (const int2*)t->d_ba_crowded, t->ba_crowded_cap);
    HIPCHK(hipEventRecord(t->ev_ba_read, s));
    HIPCHK(hipStreamWaitEvent(S.stream, t->ev_ba_read, 0));
  }
  if (int r = refStagesFromPool(t, ref_slot, s)) return r;
  int out[DMV_MAX_LEVELS + 1] = {};   // pc_n and, behind it, the number of selected residuals: one download
  HIPCHK(c->bounce.d2h(out, t->d_pc_n, sizeof(int) * (DMV_MAX_LEVELS + 1), s));
  HIPCHK(c->bounce.finish(s));
  refPublish(t, out, ref_exposure, aff_a, aff_b);
  if (n_selected) *n_selected = out[dmvio_hip_tracker::REF_BA_SELECTED];
  return 0;
}

int dmvio_hip_tracker_set_ref_from_ba_batch(dmvio_hip_set_ref_batch* b, int W, dmvio_hip_set_ref_ba_window* win) {
  // every refusal stands before the first enqueue and before the first write to a tracker
  if (int r = dmvBatchHead(b, W, b ? b->max_windows : 0, win, "tracker_set_ref_from_ba_batch", REF_HEAD_TEXT)) return r;
  dmvio_hip_ctx* c = b->ctx;
  std::vector<dmvio_hip_ba*> bas;
  for (int w = 0; w < W; w++) {
    if (!win[w].trk) return failmsg("tracker_set_ref_from_ba_batch: null tracker");
    if (!win[w].ba) return failmsg("tracker_set_ref_from_ba_batch: null BA handle");
    bas.push_back(win[w].ba);
  }
  RefBaLocks bl;
  bl.lock(bas);
  std::lock_guard<std::mutex> lk(c->mu);
  std::vector<DmvBaRefSource> S(W);
  int max_R = 0;
  for (int w = 0; w < W; w++) {
    dmv_ba_ref_source_locked(win[w].ba, &S[w]);
    if (int r = refBaCheck("tracker_set_ref_from_ba_batch", c, win[w].trk, S[w], win[w].ref_slot)) return r;
    max_R = std::max(max_R, S[w].R);
  }
  if (dmvFirstRepeated(win, W, &dmvio_hip_set_ref_ba_window::trk) >= 0)
    return failmsg("tracker_set_ref_from_ba_batch: the same tracker is named twice (two windows would write one set of buffers)");
  b->work.clear();
  if (W == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  for (int w = 0; w < W; w++) if (int r = dmv_ensure_row_major_locked(c, win[w].ref_slot)) return r;
  for (int w = 0; w < W; w++) if (int r = refBaReserve(win[w].trk, S[w].R)) return r;
  hipStream_t s = c->stream;
  RefLevels R = win[0].trk->R;   // (as in dmvio_hip_tracker_set_ref_batch: the context's geometry, the order travels in the record)
  R.order = 0;
  const int n_tiles = win[0].trk->n_tiles, flow_words = (int)win[0].trk->flow_words;
  const int n0 = R.w[0] * R.h[0];
  // the slab: two records per window, nothing else — no point crosses PCIe
  if (int r = b->slab.begin(s)) return r;
  DmvCursor L;
  const auto wins = b->slab.put<RefWin>(dmvRecords(L, sizeof(RefWin), W));
  const auto recs = b->slab.put<RefBaWin>(dmvRecords(L, sizeof(RefBaWin), W));
  RefWin* h_wins = wins.h; RefBaWin* h_bas = recs.h;
  int* const d_pcn = b->pcn.dev<int>(0); const int* const h_pcn = b->pcn.host<int>(0);
  int* d_nsel = d_pcn + (size_t)W * R.levels;
  for (int w = 0; w < W; w++) {
    dmvio_hip_tracker* t = win[w].trk;
    refWinRecord(h_wins[w], t, d_pcn + (size_t)w * R.levels, win[w].ref_slot);
    RefBaWin& A = h_bas[w];
    A.res_point = S[w].res_point; A.res_target = S[w].res_target; A.newState = S[w].newState; A.active = S[w].active; A.center = S[w].center; A.HdiF = S[w].HdiF;
    A.n_selected = d_nsel + w; A.n_crowded = t->d_pc_n + dmvio_hip_tracker::REF_BA_CROWDED; A.crowded = t->d_ba_crowded;
    A.R = S[w].R; A.newest = S[w].F - 1; A.cap = t->ba_crowded_cap; A.pad = 0;
  }
  if (int r = b->slab.upload(s, L.bytes())) return r;
  // the context's stream behind whatever the BA handles' streams still hold
  for (dmvio_hip_ba* ba : bl.held)
    for (int w = 0; w < W; w++)
      if (win[w].ba == ba) {
        HIPCHK(hipEventRecord(win[w].trk->ev_ba_ready, S[w].stream));
        HIPCHK(hipStreamWaitEvent(s, win[w].trk->ev_ba_ready, 0));
        break;
      }
  const RefWin* d_wins = wins.d; const RefBaWin* d_bas = recs.d;
  int& launches = b->work.launches;
  const unsigned gw = (unsigned)W;
  const unsigned gr = (unsigned)std::max(1, (max_R + 255) / 256);
  hipLaunchKernelGGL(k_ref_ba_clear_w, dim3((unsigned)(((n0 + 3) / 4 + 255) / 256), gw), dim3(256), 0, s, d_wins, d_bas, n0, flow_words); launches++;
  hipLaunchKernelGGL(k_ref_ba_count_w, dim3(gr, gw), dim3(256), 0, s, d_wins, d_bas, R.w[0], R.h[0]); launches++;
  hipLaunchKernelGGL(k_ref_ba_scatter_w, dim3(gr, gw), dim3(256), 0, s, d_wins, d_bas, R.w[0], R.h[0]); launches++;
  hipLaunchKernelGGL(k_ref_ba_crowded_w, dim3(gr, gw), dim3(256), 0, s, d_wins, d_bas); launches++;
  // the last read of a BA handle's arrays is behind us: their streams may go on once it has run
  hipEvent_t read = win[0].trk->ev_ba_read;
  HIPCHK(hipEventRecord(read, s));
  for (dmvio_hip_ba* ba : bl.held)
    for (int w = 0; w < W; w++)
      if (win[w].ba == ba) { HIPCHK(hipStreamWaitEvent(S[w].stream, read, 0)); break; }
  if (R.levels > 1) {
    const size_t npool = R.total - R.off[1];
    hipLaunchKernelGGL(k_ref_pool_w, dim3((unsigned)((npool + 255) / 256), gw), dim3(256), 0, s, d_wins, R); launches++;
  }
  hipLaunchKernelGGL(k_ref_dilate_w, dim3((unsigned)((R.total + 255) / 256), gw), dim3(256), 0, s, d_wins, R); launches++;
  hipLaunchKernelGGL(k_ref_count_w, dim3(n_tiles, gw), dim3(256), 0, s, d_wins, R, c->frames.built_and_waited()); launches++;
  hipLaunchKernelGGL(k_ref_scan_w, dim3(2 * R.levels, gw), dim3(1024), 0, s, d_wins, R); launches++;
  hipLaunchKernelGGL(k_ref_write_w, dim3(n_tiles, gw), dim3(256), 0, s, d_wins, R, c->frames.built_and_waited()); launches++;
  HIPCHK(hipGetLastError());
  if (int r = b->pcn.download(s, 0, sizeof(int) * (size_t)W * (R.levels + 1))) return r;   // [W][levels] pc_n, then the W selected counts
  if (int r = b->slab.wait(s)) return r;
  for (int w = 0; w < W; w++) {
    refPublish(win[w].trk, h_pcn + (size_t)w * R.levels, win[w].ref_exposure, win[w].ref_aff_a, win[w].ref_aff_b);
    win[w].n_selected = h_pcn[(size_t)W * R.levels + w];
  }
  return 0;
}

}  // extern "C"
