// ================================================================================================= window hand-over, W windows per call
// dmvio_hip_ba_set_graph_from (ba_graph_host.hpp: setGraphFrom + setGraphImpl) for W windows.  Every graph is flattened in makeIDX order straight into its section of ONE
// pinned slab the batch owns, the host tables of the single call (graphHostPrepare) are derived in place there, every handle's arena is laid out by the single call's own
// dalloc sequence (graphLayout) — the handles keep their arenas, the pointers later kernels see are the single call's — and the slab goes up in ONE copy on the batch's
// stream.  Six launches (ba_graph_batch_kernels.hpp) do for all windows what the single call enqueues per window: the arena ranges of the previous graphs cleared and the
// residual tables set to -1, the slab's pieces copied into the arenas, the Schur buckets' member lists built.  ONE wait; then the host tail.
// The slab: [W records | per window: its clear ranges, its copy pieces, then the tables in the order of GraphSection], every piece on a 256-byte granule.
// Part of capi_ba.hip's unit: included there, once, behind ba_batch_host.hpp (the batch object, its workers and events).
#pragma once
#include "ba_graph_batch_kernels.hpp"

struct GraphBatchCall {
  dmvio_hip_ba_batch* const B;
  const int W;
  const dmvio_hip_ba_graph_window* const win;
  // a window's section of the slab: byte offsets from the slab's start
  struct GraphSection {
    size_t ranges, segs, host, res_begin, point, target, u, v, color, weights, prior, idepth, top_begin, top_members, pt_first, pt_last, slot, adHost, adTarget, end;
  };
  struct Win {
    int F = 0, N = 0, R = 0, max_ranges = 0;
    GraphSection o{};
    GraphPrep G;
    unsigned long long flat_version = 0;
  };
  std::vector<Win> w;
  size_t slabBytes = 0;
  GraphBatchCall(dmvio_hip_ba_batch* B_, const int W_, const dmvio_hip_ba_graph_window* win_) : B(B_), W(W_), win(win_), w((size_t)W_) {}
  static std::string name(const int i) { return "ba_set_graph_from_batch: window " + std::to_string(i) + ": "; }
  template <class T> T* hAt(const size_t off) const { return B->graph.host<T>(off); }
  template <class T> T* dAt(const size_t off) const { return B->graph.dev<T>(off); }

  // ---- what the graphs themselves may be refused for, their sizes, the sections and the slab.  Nothing of a handle or a graph is written.
  int plan() {
    DmvCursor C;
    C.take<dmv::BAGraphWinDev>(W);
    for (int i = 0; i < W; i++) {
      const dmvio_hip_ba* b = win[i].ba;
      dmvio_hip_graph* g = win[i].graph;
      Win& q = w[i];
      {
        std::lock_guard<std::mutex> lg(g->mu);
        if ((int)g->frames.size() != b->H.F) return failmsg(name(i) + "the graph has " + std::to_string(g->frames.size()) + " keyframes, the window " + std::to_string(b->H.F));
        if (g->nDangling) return failmsg(name(i) + std::to_string(g->nDangling) + " residuals still target a removed keyframe (their dropResidual has not been forwarded)");
        if (g->nPoints < 1 || g->nRes < 1) return failmsg(name(i) + "empty graph");
        if (g->nLin > 0) return failmsg(name(i) + "the graph carries " + std::to_string(g->nLin) + " linearised residuals — dmvio_hip_ba_set_graph_from hands those over (linImport), the batched call does not");
        q.F = b->H.F; q.N = g->nPoints; q.R = g->nRes;
      }
      q.max_ranges = (int)b->arena.chunks.size() + 2;
      const size_t N = (size_t)q.N, R = (size_t)q.R, F2 = (size_t)q.F * q.F;
      GraphSection& o = q.o;
      auto take = [&C](const size_t bytes) { return C.takeBytes(bytes); };
      o.ranges = take(sizeof(dmv::BAGraphRange) * q.max_ranges); o.segs = take(sizeof(dmv::BAGraphSeg) * dmv::BA_GRAPH_MAX_SEGS);
      o.host = take(4 * N); o.res_begin = take(4 * (N + 1)); o.point = take(4 * R); o.target = take(4 * R); o.u = take(4 * N); o.v = take(4 * N);
      o.color = take(32 * N); o.weights = take(32 * N); o.prior = take(4 * N); o.idepth = take(4 * N);
      o.top_begin = take(4 * (F2 + 1)); o.top_members = take(4 * R); o.pt_first = take(4 * (size_t)q.F); o.pt_last = take(4 * (size_t)q.F); o.slot = take(4 * R);
      o.adHost = take(sizeof(double) * F2 * 64); o.adTarget = take(sizeof(double) * F2 * 64);
      o.end = C.bytes();
    }
    slabBytes = C.bytes();
    if (int r = B->graph.reserve(slabBytes, slabBytes * 2, B->stream)) return r;   // grown to twice the need and kept, like the marginalisation buffer
    if (!B->marg_ev) HIPCHK(hipEventCreateWithFlags(&B->marg_ev, hipEventDisableTiming));
    B->graph.work = &B->graph_work;
    return B->graph.begin(B->stream);
  }

  // ---- part one of the single call for window i, in the slab: the graph flattened in makeIDX order, the host tables derived beside it.  Still nothing of a handle or a
  // graph is written: a refusal here leaves every window as it was
  int prepareWindow(const int i) {
    const dmvio_hip_ba* b = win[i].ba;
    dmvio_hip_graph* g = win[i].graph;
    Win& q = w[i];
    const GraphSection& o = q.o;
    int* const host = hAt<int>(o.host); int* const res_point = hAt<int>(o.point); int* const res_target = hAt<int>(o.target);
    float* const u = hAt<float>(o.u); float* const v = hAt<float>(o.v); float* const idepth = hAt<float>(o.idepth); float* const prior = hAt<float>(o.prior);
    float* const color = hAt<float>(o.color); float* const weights = hAt<float>(o.weights);
    const float fixPrior = b->H.S.idepthFixPrior;
    {
      std::lock_guard<std::mutex> lg(g->mu);
      if ((int)g->frames.size() != q.F || g->nPoints != q.N || g->nRes != q.R || g->nDangling || g->nLin > 0) return failmsg(name(i) + "the graph was changed while the call ran");
      q.flat_version = g->version;
      int pi = 0, ri = 0;
      for (int f = 0; f < q.F; f++)
        for (const DmvGraphPoint& P : g->frames[f]) {
          host[pi] = f; u[pi] = P.u; v[pi] = P.v; idepth[pi] = P.idepth; prior[pi] = P.prior ? fixPrior : 0.0f;   // EFPoint::takeData
          memcpy(color + 8 * (size_t)pi, P.color, sizeof(P.color)); memcpy(weights + 8 * (size_t)pi, P.weights, sizeof(P.weights));
          for (int k = 0; k < P.nres; k++, ri++) { res_point[ri] = pi; res_target[ri] = P.target[k]; }
          pi++;
        }
    }
    const GraphLists L{hAt<int>(o.res_begin), hAt<int>(o.top_begin), hAt<int>(o.top_members), hAt<int>(o.pt_first), hAt<int>(o.pt_last), hAt<int>(o.slot)};
    if (graphHostPrepare(q.F, q.N, host, q.R, res_point, res_target, L, q.G)) return failmsg(name(i) + dmv_err());
    if (!q.G.scd_on_device)
      return failmsg(name(i) + "a point observes one keyframe twice — dmvio_hip_ba_set_graph_from serves such a graph (Schur lists built on the host), the batched call does not");
    return 0;
  }

  // ---- every window is valid: the handle's part of the single call up to its enqueue — the old graph dropped, the host mirrors, the arena laid out (part two) — and the
  // window's record, clear ranges and copy pieces
  int layoutWindow(const int i) {
    dmvio_hip_ba* b = win[i].ba;
    Win& q = w[i];
    const GraphSection& o = q.o;
    const int N = q.N, R = q.R, F = q.F, F2 = F * F;
    b->stateChanged();
    graphDropOld(b);
    const std::vector<size_t> prevUsed = b->arena.used;   // what the previous graph used of every chunk: cleared by k_ba_graph_clear_b
    std::fill(b->arena.used.begin(), b->arena.used.end(), (size_t)0);
    b->h_host.assign(hAt<int>(o.host), hAt<int>(o.host) + N); b->h_point.assign(hAt<int>(o.point), hAt<int>(o.point) + R); b->h_target.assign(hAt<int>(o.target), hAt<int>(o.target) + R);
    b->h_res_begin.assign(hAt<int>(o.res_begin), hAt<int>(o.res_begin) + N + 1);
    b->h_newest.swap(q.G.newest);
    // (graphLayout replaces a grow-only pinned buffer that has become too small; kernels still pending on the handle's own stream may store into the old one)
    if ((size_t)N > b->cap_idepth_backup || (size_t)2 * ((N + 255) / 256) > b->cap_spart) HIPCHK(hipStreamSynchronize(b->stream));
    GraphDev D;
    if (int r = graphLayout(b, q.G, D)) return r;
    b->graphReplaced();
    // the adjoint tables as they stand (uploadAdjoints of the single call)
    if (b->H.adHost.size() != (size_t)F2 * 64 || b->H.adTarget.size() != (size_t)F2 * 64) return failmsg(name(i) + "adjoint tables of an unexpected size");
    memcpy(hAt<char>(o.adHost), b->H.adHost.data(), sizeof(double) * F2 * 64); memcpy(hAt<char>(o.adTarget), b->H.adTarget.data(), sizeof(double) * F2 * 64);
    b->adj_dirty = false;
    // ---- clear ranges: [0, used) of every chunk, minus the new residual table, which is filled with -1 instead
    dmv::BAGraphRange* const rg = hAt<dmv::BAGraphRange>(o.ranges);
    int nr = 0;
    char* const ridx = reinterpret_cast<char*>(D.ridx);
    const size_t ridxBytes = (sizeof(int) * (size_t)N * F + 15) & ~(size_t)15;
    auto range = [&](char* p, const size_t bytes, const unsigned int value) {
      if (bytes) { rg[nr].p = reinterpret_cast<uint4*>(p); rg[nr].n16 = bytes / 16; rg[nr].value = value; rg[nr].pad = 0; nr++; }
    };
    for (size_t k = 0; k < prevUsed.size(); k++) {
      char* const base = b->arena.chunks[k].first;
      const size_t used = prevUsed[k];
      if (ridx >= base && ridx < base + b->arena.chunks[k].second) {
        const size_t r0 = (size_t)(ridx - base), r1 = r0 + ridxBytes;
        range(base, std::min(used, r0), 0u);
        if (used > r1) range(base + r1, used - r1, 0u);
      } else range(base, used, 0u);
    }
    range(ridx, ridxBytes, 0xffffffffu);
    if (nr > q.max_ranges) return failmsg(name(i) + "more clear ranges than planned");
    // ---- copy pieces
    dmv::BAGraphSeg* const sg = hAt<dmv::BAGraphSeg>(o.segs);
    int ns = 0;
    auto piece = [&](void* dst, const size_t src, const size_t bytes) {
      sg[ns].dst = reinterpret_cast<uint4*>(dst); sg[ns].src = dAt<const uint4>(src); sg[ns].n16 = (bytes + 15) / 16; ns++;
    };
    piece(D.host, o.host, 4 * (size_t)N); piece(D.res_begin, o.res_begin, 4 * ((size_t)N + 1)); piece(D.point, o.point, 4 * (size_t)R); piece(D.target, o.target, 4 * (size_t)R);
    piece(D.u, o.u, 4 * (size_t)N); piece(D.v, o.v, 4 * (size_t)N); piece(D.color, o.color, 32 * (size_t)N); piece(D.weights, o.weights, 32 * (size_t)N);
    piece(D.prior, o.prior, 4 * (size_t)N); piece(b->P.idepth, o.idepth, 4 * (size_t)N); piece(b->P.idepth_zero, o.idepth, 4 * (size_t)N);
    piece(b->d_top_begin, o.top_begin, 4 * ((size_t)F2 + 1)); piece(b->d_top_members, o.top_members, 4 * (size_t)R);
    piece(D.first, o.pt_first, 4 * (size_t)F); piece(D.last, o.pt_last, 4 * (size_t)F); piece(b->d_newestSlot, o.slot, 4 * (size_t)R);
    piece(b->d_adHost, o.adHost, sizeof(double) * F2 * 64); piece(b->d_adTarget, o.adTarget, sizeof(double) * F2 * 64);
    static_assert(18 <= dmv::BA_GRAPH_MAX_SEGS, "a window's copy pieces");
    // ---- the record
    dmv::BAGraphWinDev& V = hAt<dmv::BAGraphWinDev>(0)[i];
    memset(&V, 0, sizeof(V));
    V.F = F; V.N = N; V.R = R; V.n_ranges = nr; V.n_segs = ns;
    V.ranges = dAt<const dmv::BAGraphRange>(o.ranges); V.segs = dAt<const dmv::BAGraphSeg>(o.segs);
    V.point = D.point; V.target = D.target; V.host = D.host; V.pt_first = D.first; V.pt_last = D.last;
    V.ridx = D.ridx; V.cnt = D.cnt; V.scd_begin = b->d_scd_begin; V.scd_members = b->d_scd_members;
    return 0;
  }

  int enqueue() {
    const hipStream_t s = B->stream;
    DmvWork& work = B->graph_work;
    // a handle's own stream may still hold work (its entry points return on a ticket, not on an empty stream): in front of the call
    for (int i = 0; i < W; i++) {
      dmvio_hip_ba* b = win[i].ba;
      if (b->stream == s || hipStreamQuery(b->stream) == hipSuccess) continue;
      HIPCHK(hipEventRecord(B->marg_ev, b->stream));
      HIPCHK(hipStreamWaitEvent(s, B->marg_ev, 0));
    }
    (void)hipGetLastError();   // (hipErrorNotReady of the query above is no error)
    if (B->profile) HIPCHK(hipEventRecord(B->ev[6], s));
    if (int r = B->graph.upload(s, slabBytes)) return r;
    // grid extents: the largest window's
    unsigned long long clear16 = 1, piece16 = 1;
    int Rmax = 1, Fmax = 1;
    const dmv::BAGraphWinDev* const hw = hAt<const dmv::BAGraphWinDev>(0);
    for (int i = 0; i < W; i++) {
      unsigned long long c = 0;
      const dmv::BAGraphRange* rg = hAt<const dmv::BAGraphRange>(w[i].o.ranges);
      for (int k = 0; k < hw[i].n_ranges; k++) c = std::max(c, rg[k].n16);
      clear16 = std::max(clear16, c);
      const dmv::BAGraphSeg* sg = hAt<const dmv::BAGraphSeg>(w[i].o.segs);
      for (int k = 0; k < hw[i].n_segs; k++) piece16 = std::max(piece16, sg[k].n16);
      Rmax = std::max(Rmax, w[i].R); Fmax = std::max(Fmax, w[i].F);
    }
    // clear: a thread takes sixteen 16-byte stores of the largest range, up to 256 workgroups per window (grid-stride beyond); copy: one per thread, up to 32 workgroups
    const int gx_clear = (int)std::min<unsigned long long>(256, (clear16 + 256 * 16 - 1) / (256 * 16));
    const int gx_piece = (int)std::min<unsigned long long>(32, (piece16 + 255) / 256);
    const dmv::BAGraphWinDev* const dw = dAt<const dmv::BAGraphWinDev>(0);
    hipLaunchKernelGGL(dmv::k_ba_graph_clear_b, dim3(gx_clear, W), dim3(256), 0, s, dw); work.launches++;
    hipLaunchKernelGGL(dmv::k_ba_graph_scatter_b, dim3(gx_piece, W), dim3(256), 0, s, dw); work.launches++;
    hipLaunchKernelGGL(dmv::k_ba_scd_ridx_b, dim3((Rmax + 255) / 256, W), dim3(256), 0, s, dw); work.launches++;
    const int gx_lists = Fmax * ((Fmax * Fmax + 3) / 4);
    hipLaunchKernelGGL(dmv::k_ba_scd_lists_b, dim3(gx_lists, W), dim3(256), 0, s, dw, 0); work.launches++;
    hipLaunchKernelGGL(dmv::k_ba_scd_scan_b, dim3(1, W), dim3(1024), 0, s, dw); work.launches++;
    hipLaunchKernelGGL(dmv::k_ba_scd_lists_b, dim3(gx_lists, W), dim3(256), 0, s, dw, 1); work.launches++;
    HIPCHK(hipGetLastError());
    if (B->profile) HIPCHK(hipEventRecord(B->ev[7], s));
    if (int r = B->graph.wait(s)) return r;
    B->graph_ms = 0;
    if (B->profile) HIPCHK(hipEventElapsedTime(&B->graph_ms, B->ev[6], B->ev[7]));
    return 0;
  }

  // ---- behind the wait (the handle's own stream is drained with it): the host-coherent record cleared as the single call clears it, the window ready, the graph's flat
  // order the one dmvio_hip_graph_set_idepths accepts values in
  int finishWindow(const int i) {
    dmvio_hip_ba* b = win[i].ba;
    memset(b->h_res, 0, sizeof(BAHostRes));
    b->graph_ready = true;
    std::lock_guard<std::mutex> lg(win[i].graph->mu);
    win[i].graph->flat_version = w[i].flat_version;
    return 0;
  }
};

extern "C" {
int dmvio_hip_ba_set_graph_from_batch(dmvio_hip_ba_batch* B, int W, const dmvio_hip_ba_graph_window* win) {
  if (!B) return failmsg("ba_set_graph_from_batch: null batch");
  if (W < 0) return failmsg("ba_set_graph_from_batch: W < 0");
  if (W > B->cap) return failmsg("ba_set_graph_from_batch: more windows than the batch was created for");
  std::lock_guard<std::mutex> lkB(B->mu);
  if (W == 0) { B->graph_work.clear(); B->graph_ms = 0; return 0; }
  if (!win) return failmsg("ba_set_graph_from_batch: null window list");
  std::vector<dmvio_hip_ba*> order(W);
  for (int i = 0; i < W; i++) {
    if (!win[i].ba) return failmsg(GraphBatchCall::name(i) + "null handle");
    if (!win[i].graph) return failmsg(GraphBatchCall::name(i) + "null graph");
    if (win[i].ba->ctx != B->ctx) return failmsg(GraphBatchCall::name(i) + "the handle belongs to another context");
    order[i] = win[i].ba;
  }
  // the handles' locks, in address order (as dmvio_hip_ba_marginalize_points_batch)
  if (const int j = dmvFirstRepeated(win, W, &dmvio_hip_ba_graph_window::ba); j >= 0) return failmsg(GraphBatchCall::name(j) + "its handle appears twice in the call");
  std::sort(order.begin(), order.end());
  std::vector<std::unique_lock<std::recursive_mutex>> locks;
  for (dmvio_hip_ba* b : order) locks.emplace_back(b->mu);
  for (int i = 0; i < W; i++) {
    if (win[i].ba->H.F < 1) return failmsg(GraphBatchCall::name(i) + "a handle without a window (dmvio_hip_ba_set_window first)");
    if (sharded(win[i].ba)) return failmsg(GraphBatchCall::name(i) + "a window sharded over ranks cannot join a batch");
  }
  HIPCHK(hipSetDevice(B->ctx->device));
  GraphBatchCall c(B, W, win);
  if (int r = c.plan()) return r;
  if (int r = B->workers.parallelFor(W, [&c](const int i) { return c.prepareWindow(i); })) return r;
  // from here on the handles change
  B->graph_work.clear();
  if (int r = B->workers.parallelFor(W, [&c](const int i) { return c.layoutWindow(i); })) return r;
  if (int r = c.enqueue()) return r;
  return B->workers.parallelFor(W, [&c](const int i) { return c.finishWindow(i); });
}
int dmvio_hip_ba_batch_last_graph_work(dmvio_hip_ba_batch* B, int* launches, int* uploads, int* downloads, int* waits) {
  if (!B) return failmsg("ba_batch_last_graph_work: null batch");
  std::lock_guard<std::mutex> lkB(B->mu);
  B->graph_work.report(launches, uploads, downloads, waits);
  return 0;
}
int dmvio_hip_ba_batch_last_graph_ms(dmvio_hip_ba_batch* B, float* ms) {
  if (!B || !ms) return failmsg("ba_batch_last_graph_ms: null argument");
  std::lock_guard<std::mutex> lkB(B->mu);
  *ms = B->graph_ms;
  return 0;
}
}  // extern "C"
