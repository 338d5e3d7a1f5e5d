// Building the window's device graph: dmvio_hip_ba_set_graph (flat arrays) and dmvio_hip_ba_set_graph_from (the resident mirror, capi_graph.hip), and the buffers of residuals
// kept linearised (first use, hand-over, the host copies the energy term reads).  The build is three parts — the host preparation (graphHostPrepare), the arena layout
// (graphLayout) and the enqueue — of which the batched hand-over (ba_graph_batch_host.hpp) shares the first two.  A declaration file of capi_ba.hip's translation unit: included there, once, behind dalloc /
// freeDevice / uploadAdjoints and ba_shard_host.hpp.
#pragma once
// ---- part one: the host preparation.  Validation and every table the host derives from the flat arrays, written where the caller wants them (the single call: vectors of
// its own; the batched hand-over, ba_graph_batch_host.hpp: the window's section of the pinned slab).  Touches no handle.
struct GraphLists {   // destinations: res_begin N + 1, top_begin F*F + 1, top_members R, pt_first / pt_last F, slot R
  int *res_begin, *top_begin, *top_members, *pt_first, *pt_last, *slot;
};
struct GraphPrep {
  int F = 0, N = 0, R = 0;
  size_t npairs = 0;
  bool scd_on_device = true;                 // no point observes a keyframe twice: the Schur buckets' member lists are built on the device
  std::vector<int> newest;                   // residuals that target the newest keyframe, ascending
  std::vector<int> scd_begin, scd_members;   // the host-built lists (!scd_on_device)
};
static int graphHostPrepare(const int F, const int N, const int* host, const int R, const int* res_point, const int* res_target, const GraphLists& L, GraphPrep& G) {
  const int F2 = F * F;
  G.F = F; G.N = N; G.R = R;
  G.newest.clear();
  for (int ri = 0; ri < R; ri++) if (res_target[ri] == F - 1) G.newest.push_back(ri);
  // residuals must be grouped by point, points in window order
  int* const res_begin = L.res_begin;
  std::fill(res_begin, res_begin + N + 1, 0);
  for (int ri = 0; ri < R; ri++) {
    const int p = res_point[ri];
    if (p < 0 || p >= N || res_target[ri] < 0 || res_target[ri] >= F) return failmsg("ba_set_graph: residual index out of range");
    if (ri > 0 && p < res_point[ri - 1]) return failmsg("ba_set_graph: residuals must be sorted by point");
    if (host[p] < 0 || host[p] >= F || host[p] == res_target[ri]) return failmsg("ba_set_graph: bad host / target");
    res_begin[p + 1]++;
  }
  for (int p = 0; p < N; p++) res_begin[p + 1] += res_begin[p];
  // bucket member lists in the reference's traversal order (points, then residuals of the point)
  int* const top_begin = L.top_begin;
  std::fill(top_begin, top_begin + F2 + 1, 0);
  for (int ri = 0; ri < R; ri++) top_begin[host[res_point[ri]] + F * res_target[ri] + 1]++;
  for (int k = 0; k < F2; k++) top_begin[k + 1] += top_begin[k];
  { std::vector<int> cur(top_begin, top_begin + F2); for (int ri = 0; ri < R; ri++) L.top_members[cur[host[res_point[ri]] + F * res_target[ri]]++] = ri; }
  G.npairs = 0;
  for (int p = 0; p < N; p++) { const size_t k = res_begin[p + 1] - res_begin[p]; G.npairs += k * k; }
  // The Schur buckets' member lists are built on the device (k_ba_scd_*: ba_kernels.hpp) when no point observes a keyframe twice — always, in the reference's graphs (one
  // PointFrameResidual per point and target, FullSystem.cpp:1248-1262); a graph that does is served by the host loops below, as every graph was before.
  std::fill(L.pt_first, L.pt_first + F, N); std::fill(L.pt_last, L.pt_last + F, -1);
  G.scd_on_device = true;
  for (int p = 0; p < N && G.scd_on_device; p++) {
    L.pt_first[host[p]] = std::min(L.pt_first[host[p]], p); L.pt_last[host[p]] = std::max(L.pt_last[host[p]], p);
    unsigned int seen = 0;
    for (int ri = res_begin[p]; ri < res_begin[p + 1]; ri++) { const unsigned int bit = 1u << res_target[ri]; if (seen & bit) G.scd_on_device = false; seen |= bit; }
  }
  G.scd_begin.clear(); G.scd_members.clear();
  if (!G.scd_on_device) {
    G.scd_begin.assign(F2 * F + 1, 0); G.scd_members.resize(3 * G.npairs);
    for (int p = 0; p < N; p++)
      for (int r1 = res_begin[p]; r1 < res_begin[p + 1]; r1++)
        for (int r2 = res_begin[p]; r2 < res_begin[p + 1]; r2++) G.scd_begin[(host[p] + F * res_target[r1]) + res_target[r2] * F2 + 1]++;
    for (int k = 0; k < F2 * F; k++) G.scd_begin[k + 1] += G.scd_begin[k];
    std::vector<int> cur(G.scd_begin.begin(), G.scd_begin.end() - 1);
    for (int p = 0; p < N; p++)
      for (int r1 = res_begin[p]; r1 < res_begin[p + 1]; r1++)
        for (int r2 = res_begin[p]; r2 < res_begin[p + 1]; r2++) {
          const int k = (host[p] + F * res_target[r1]) + res_target[r2] * F2;
          const int o = cur[k]++;
          G.scd_members[3 * o] = r1; G.scd_members[3 * o + 1] = r2; G.scd_members[3 * o + 2] = p;
        }
  }
  // per residual: its position among the residuals that target the newest keyframe, or -1
  std::fill(L.slot, L.slot + R, -1);
  for (size_t k = 0; k < G.newest.size(); k++) L.slot[G.newest[k]] = (int)k;
  return 0;
}
// what a new graph does to the handle before anything of it exists: the arrays outside the arena go, and so does everything the old graph's linearised residuals left
// behind (residuals kept linearised belong to the graph they were linearised in)
static void graphDropOld(dmvio_hip_ba* b) {
  b->th_pending = false;   // the stream is drained and h_res is cleared (th_ticket restarts at 0 while b->ticket keeps counting): nothing of the old graph may be awaited
  freeDevice(b);
  b->n_lin = 0; b->n_lin_global = 0; b->Rs.lin = nullptr; b->P.lHdd = b->P.lbd = b->P.lHcd = nullptr; b->P.HcdAF = nullptr; b->d_lin = nullptr; b->d_red1 = nullptr; b->H.HLraw.clear(); b->H.bLraw.clear();
  b->h_lin.clear(); b->h_linAct.clear(); b->h_linJ.clear(); b->h_rtz.clear(); b->fullJ_applied = false;
}
// ---- part two: the arena layout — the dalloc sequence of a graph of N points / R residuals in a window of F keyframes, from the start of the (cleared) arena; with it the
// handle's kernel views, grid sizes and grow-only pinned buffers (the host mirrors are in place by now: h_newest sizes d_newestE).  The arrays that receive uploads come
// back in GraphDev.
struct GraphDev {
  int *host, *res_begin, *point, *target;
  float *u, *v, *color, *weights, *prior;
  int *ridx, *cnt, *first, *last;   // scd_on_device only
};
static int graphLayout(dmvio_hip_ba* b, const GraphPrep& G, GraphDev& D) {
  const int N = G.N, R = G.R, F = G.F, F2 = F * F;
  b->arena.cur = 0; b->arena.off = 0;
  struct ArenaScope { dmvio_hip_ba* b; ~ArenaScope() { b->arena.on = false; } } arenaScope{b};
  b->arena.on = true;
  b->H.N = N; b->H.R = R;
  if (dalloc(b, &D.host, N) || dalloc(b, &D.res_begin, N + 1) || dalloc(b, &D.point, R) || dalloc(b, &D.target, R) || dalloc(b, &D.u, N) || dalloc(b, &D.v, N) ||
      dalloc(b, &D.color, (size_t)N * 8) || dalloc(b, &D.weights, (size_t)N * 8) || dalloc(b, &D.prior, N)) return -1;
  BAPoints& P = b->P; BARes& Rs = b->Rs;
  if (dalloc(b, &P.idepth, N) || dalloc(b, &P.idepth_zero, N) || dalloc(b, &P.idepth_backup, N) || dalloc(b, &P.step, N) || dalloc(b, &P.Hdd, N) || dalloc(b, &P.bd, N) ||
      dalloc(b, &P.Hcd, (size_t)N * 4) || dalloc(b, &P.HdiF, N) || dalloc(b, &P.bdSumF, N) || dalloc(b, &P.idepth_hessian, N) ||
      dalloc(b, &b->d_cand, N) || dalloc(b, &b->d_decision, N) || dalloc(b, &b->d_mHdiF, N) || dalloc(b, &b->d_mbdSumF, N) || dalloc(b, &b->d_mHcd, (size_t)N * 4) ||
      dalloc(b, &b->d_margRec, (size_t)R * REC_FLOATS) || dalloc(b, &b->d_margActive, R) || dalloc(b, &b->d_adHTdelta, (size_t)F2 * 8)) return -1;
  if (dalloc(b, &Rs.removed, R) || dalloc(b, &Rs.state, R) || dalloc(b, &Rs.newState, R) || dalloc(b, &Rs.active, R) || dalloc(b, &Rs.which, R) || dalloc(b, &Rs.energy, R) || dalloc(b, &Rs.newEnergy, R) ||
      dalloc(b, &Rs.center, (size_t)R * 3) || dalloc(b, &Rs.rec[0], (size_t)R * REC_FLOATS) || dalloc(b, &Rs.rec[1], (size_t)R * REC_FLOATS)) return -1;
  P.host = D.host; P.u = D.u; P.v = D.v; P.color = D.color; P.weights = D.weights; P.priorF = D.prior; P.res_begin = D.res_begin;
  Rs.point = D.point; Rs.target = D.target;
  if (dalloc(b, &b->d_pre, (size_t)F2) || dalloc(b, &b->d_adHost, (size_t)F2 * 64) || dalloc(b, &b->d_adTarget, (size_t)F2 * 64) || dalloc(b, &b->d_top_begin, F2 + 1) ||
      dalloc(b, &b->d_top_members, R) || dalloc(b, &b->d_scd_begin, F2 * F + 1) || dalloc(b, &b->d_scd_members, 3 * G.npairs) || dalloc(b, &b->d_accTop, (size_t)F2 * 96 * b->nsTop) ||
      dalloc(b, &b->d_accD, (size_t)F2 * F * 64 * b->nsD) || dalloc(b, &b->d_accE, (size_t)F2 * 40 * b->nsTop) || dalloc(b, &b->d_accC, 20 * b->nsC) || dalloc(b, &b->d_numTop, F2 * b->nsTop) || dalloc(b, &b->d_numD, F2 * F * b->nsD)) return -1;
  D.ridx = D.cnt = D.first = D.last = nullptr;
  if (G.scd_on_device) { if (dalloc(b, &D.ridx, (size_t)N * F) || dalloc(b, &D.cnt, (size_t)F2 * F) || dalloc(b, &D.first, F) || dalloc(b, &D.last, F)) return -1; }
  StitchBufs& SB = b->SB;
  if (dalloc(b, &SB.topHH, (size_t)F * 64) || dalloc(b, &SB.topTT, (size_t)F2 * 64) || dalloc(b, &SB.topHT, (size_t)F2 * 64) || dalloc(b, &SB.topHC, (size_t)F * 32) ||
      dalloc(b, &SB.topTC, (size_t)F2 * 32) || dalloc(b, &SB.topBH, (size_t)F * 8) || dalloc(b, &SB.topBT, (size_t)F2 * 8) || dalloc(b, &SB.topCC, (size_t)F * 20) ||
      dalloc(b, &SB.scHH, (size_t)F2 * 64) || dalloc(b, &SB.scTT, (size_t)F2 * F * 64) || dalloc(b, &SB.scTH, (size_t)F2 * 64) || dalloc(b, &SB.scHT, (size_t)F2 * F * 64) ||
      dalloc(b, &SB.scHC, (size_t)F2 * 32) ||
      dalloc(b, &SB.scTC, (size_t)F2 * 32) || dalloc(b, &SB.scBH, (size_t)F2 * 8) || dalloc(b, &SB.scBT, (size_t)F2 * 8)) return -1;
  const int n = b->H.n(), tot = 2 * (n * n + n);
  b->n_lin_blocks = (R + LIN_RES_PER_BLOCK - 1) / LIN_RES_PER_BLOCK; b->n_pt_blocks = (N + 255) / 256; b->n_pt8_blocks = (N + PT_GROUPS_PER_BLOCK - 1) / PT_GROUPS_PER_BLOCK;
  // energy partials (doubles) and the per-residual energies with outliers (floats) share one pinned allocation the kernel stores into
  b->n_epart = std::max(b->n_lin_blocks, F2 * 8);
  if (dalloc(b, &b->d_spart, 2 * b->n_pt_blocks) || dalloc(b, &b->d_fullJ, (size_t)R * FJ_FLOATS)) return -1;
  // what the host reads back every iteration (the stitched system, the energy partials, the per-residual energies) is written by the
  // kernels straight into pinned host memory (h_sys, h_res: allocated with the handle, sized for BA_MAXF_CAP keyframes): no copy engine between the last kernel and the host's wait
  if (dalloc(b, &b->d_sys, (size_t)tot + 1)) return -1;
  b->xchg_width = 0; b->d_xchg_local = b->d_xchg_all = nullptr;
  if ((size_t)N > b->cap_idepth_backup) {
    if (b->h_idepth_backup) HIPCHK(hipHostFree(b->h_idepth_backup));
    b->cap_idepth_backup = (size_t)N + (size_t)N / 2 + 256;
    HIPCHK(hipHostMalloc((void**)&b->h_idepth_backup, sizeof(float) * b->cap_idepth_backup, hipHostMallocCoherent | hipHostMallocMapped));
  }
  if (dalloc(b, &b->d_ctl, 1) || dalloc(b, &b->d_frameTH, BA_MAXF_CAP) || dalloc(b, &b->d_epart, (size_t)b->n_epart) || dalloc(b, &b->d_newestSlot, (size_t)R) || dalloc(b, &b->d_newestE, b->h_newest.size()) ||
      dalloc(b, &b->d_newEnergyWO, (size_t)R)) return -1;
  Rs.newestSlot = b->d_newestSlot; Rs.newestE = b->d_newestE;
  Rs.newEnergyWO = b->d_newEnergyWO;
  if ((size_t)2 * b->n_pt_blocks > b->cap_spart) {
    if (b->h_spart) HIPCHK(hipHostFree(b->h_spart));
    b->cap_spart = (size_t)2 * b->n_pt_blocks + 64;
    HIPCHK(hipHostMalloc((void**)&b->h_spart, sizeof(float) * b->cap_spart, hipHostMallocDefault));
  }
  return 0;
}
// ---- the single call: parts one and two, then part three, the enqueue on the handle's own stream
static int setGraphImpl(dmvio_hip_ba* b, int N, const int* host, const float* u, const float* v, const float* idepth, const float* color8,
                        const float* weights8, const unsigned char* hasDepthPrior, int R, const int* res_point, const int* res_target, bool wait) {
  if (!b || !host || !u || !v || !idepth || !color8 || !weights8 || !res_point || !res_target) return failmsg("ba_set_graph: null argument");
  BA_LOCK(b);
  b->stateChanged();
  BAHost& H = b->H;
  if (H.F < 1) return failmsg("ba_set_graph: set_window first");
  if (N < 1 || R < 1) return failmsg("ba_set_graph: empty graph");
  dmvio_hip_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->device));
  double tg0 = b->timing ? nowUs() : 0, tg1;
#define SG_PH(i) do { if (b->timing) { tg1 = nowUs(); b->tm_graph[i] += tg1 - tg0; tg0 = tg1; } } while (0)
  HIPCHK(hipStreamSynchronize(b->stream));
  graphDropOld(b);
  // the arena of the previous graph, cleared for this one on the handle's stream; the uploads and kernels below follow on the same stream: no wait
  for (size_t k = 0; k < b->arena.chunks.size(); k++) if (b->arena.used[k]) { HIPCHK(hipMemsetAsync(b->arena.chunks[k].first, 0, b->arena.used[k], b->stream)); b->arena.used[k] = 0; }   // what the previous graph used, not the whole chunk
  SG_PH(0);
  const int F = H.F, F2 = F * F;
  H.N = N; H.R = R;
  std::vector<int> res_begin(N + 1), top_begin(F2 + 1), top_members(R), pt_first(F), pt_last(F), slot(R);
  GraphPrep G;
  if (int r = graphHostPrepare(F, N, host, R, res_point, res_target, GraphLists{res_begin.data(), top_begin.data(), top_members.data(), pt_first.data(), pt_last.data(), slot.data()}, G)) return r;
  b->h_host.assign(host, host + N); b->h_point.assign(res_point, res_point + R); b->h_target.assign(res_target, res_target + R);
  b->h_newest.swap(G.newest);
  b->h_res_begin.swap(res_begin);
  SG_PH(1);
  // ---- device arrays
  GraphDev D;
  if (int r = graphLayout(b, G, D)) return r;
  BAPoints& P = b->P;
  std::vector<float> prior(N, 0.0f);
  if (hasDepthPrior) for (int p = 0; p < N; p++) prior[p] = hasDepthPrior[p] ? H.S.idepthFixPrior : 0.0f;   // EFPoint::takeData
  hipStream_t s = b->stream;
  SG_PH(2);
  // the uploads of this call are staged and leave merged (DmvBounce::begin_group): the nine point / residual tables and the two copies of idepth are one copy, ...
  struct GroupScope { DmvBounce& bn; ~GroupScope() { bn.grouping = false; bn.group.clear(); } } groupScope{b->bounce};   // an error return drops what was only staged
  b->bounce.begin_group();
  HIPCHK(b->bounce.h2d(D.host, host, sizeof(int) * N, s));
  HIPCHK(b->bounce.h2d(D.res_begin, b->h_res_begin.data(), sizeof(int) * (N + 1), s));
  HIPCHK(b->bounce.h2d(D.point, res_point, sizeof(int) * R, s));
  HIPCHK(b->bounce.h2d(D.target, res_target, sizeof(int) * R, s));
  HIPCHK(b->bounce.h2d(D.u, u, sizeof(float) * N, s));
  HIPCHK(b->bounce.h2d(D.v, v, sizeof(float) * N, s));
  HIPCHK(b->bounce.h2d(D.color, color8, sizeof(float) * N * 8, s));
  HIPCHK(b->bounce.h2d(D.weights, weights8, sizeof(float) * N * 8, s));
  HIPCHK(b->bounce.h2d(D.prior, prior.data(), sizeof(float) * N, s));
  HIPCHK(b->bounce.h2d(P.idepth, idepth, sizeof(float) * N, s));
  HIPCHK(b->bounce.h2d(P.idepth_zero, idepth, sizeof(float) * N, s));
  HIPCHK(b->bounce.h2d(b->d_top_begin, top_begin.data(), sizeof(int) * (F2 + 1), s));
  HIPCHK(b->bounce.h2d(b->d_top_members, top_members.data(), sizeof(int) * R, s));
  if (!G.scd_on_device) {
    HIPCHK(b->bounce.h2d(b->d_scd_begin, G.scd_begin.data(), sizeof(int) * (F2 * F + 1), s));
    HIPCHK(b->bounce.h2d(b->d_scd_members, G.scd_members.data(), sizeof(int) * 3 * G.npairs, s));
    HIPCHK(b->bounce.end_group(s));
  } else {
    // behind the uploads of host / point / target on the same stream: residual table, counts, scan, members
    HIPCHK(b->bounce.h2d(D.first, pt_first.data(), sizeof(int) * F, s));
    HIPCHK(b->bounce.h2d(D.last, pt_last.data(), sizeof(int) * F, s));
    HIPCHK(b->bounce.end_group(s));   // the kernels below read what was staged so far
    HIPCHK(hipMemsetAsync(D.ridx, 0xff, sizeof(int) * (size_t)N * F, s));
    hipLaunchKernelGGL(k_ba_scd_ridx, dim3((R + 255) / 256), dim3(256), 0, s, R, F, (const int*)D.point, (const int*)D.target, D.ridx);
    hipLaunchKernelGGL(k_ba_scd_lists, dim3((F2 + 3) / 4, F), dim3(256), 0, s, F, (const int*)D.first, (const int*)D.last, (const int*)D.host, (const int*)D.ridx, 0, D.cnt, (const int*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(k_ba_scd_scan, dim3(1), dim3(1024), 0, s, F2 * F, (const int*)D.cnt, b->d_scd_begin);
    hipLaunchKernelGGL(k_ba_scd_lists, dim3((F2 + 3) / 4, F), dim3(256), 0, s, F, (const int*)D.first, (const int*)D.last, (const int*)D.host, (const int*)D.ridx, 1, D.cnt, (const int*)b->d_scd_begin, b->d_scd_members);
    HIPCHK(hipGetLastError());
  }
  SG_PH(3);
  b->bounce.begin_group();   // ... the slot table and the adjoint tables another
  b->graphReplaced();
  memset(b->h_res, 0, sizeof(BAHostRes));
  HIPCHK(b->bounce.h2d(b->d_newestSlot, slot.data(), sizeof(int) * R, s));   // staged (the vector may go): asynchronous like the other uploads
  SG_PH(4);
  if (int r = uploadAdjoints(b)) return r;
  HIPCHK(b->bounce.end_group(s));
  // everything above is staged in pinned memory and enqueued on the handle's stream, and so is whatever uses it: dmvio_hip_ba_set_graph_from does not wait (the 0.1 ms the
  // uploads take overlap the caller's next calls — frame states, prior, the first host-side steps of optimize)
  HIPCHK(hipGetLastError());
  if (wait) HIPCHK(hipStreamSynchronize(s));
  SG_PH(5);
#undef SG_PH
  b->tm_graph_n++;
  b->graph_ready = true;
  return 0;
}
// buffers of the residuals kept linearised (first use on a graph)
static int linAlloc(dmvio_hip_ba* b) {
  const int R = b->H.R, N = b->H.N;
  if (b->d_lin) return 0;
  if (dalloc(b, &b->d_lin, R) || dalloc(b, &b->d_linMask, R) || dalloc(b, &b->d_linActive, R) || dalloc(b, &b->d_topActive, R) || dalloc(b, &b->d_rtz, (size_t)R * 8) ||
      dalloc(b, &b->d_linRec, (size_t)R * REC_FLOATS) || dalloc(b, &b->d_lHdd, N) || dalloc(b, &b->d_lbd, N) || dalloc(b, &b->d_lHcd, (size_t)N * 4) ||
      dalloc(b, &b->d_HcdAF, (size_t)N * 4) || dalloc(b, &b->d_linE, (size_t)R * 8)) return -1;
  b->h_lin.assign(R, 0);
  HIPCHK(hipMemsetAsync(b->d_lin, 0, R, b->stream));   // (the arena hands out zeroed memory after set_graph; a second graph's first use must not depend on it)
  return 0;
}
// after the device flags changed: the host copies calcLEnergyPt reads (the energy terms are host arithmetic in this library), the counts, the kernels' views
static int linFinish(dmvio_hip_ba* b, int* n_linearized) {
  const int R = b->H.R;
  hipStream_t s = b->stream;
  b->h_linAct.resize(R); b->h_linJ.resize((size_t)R * FJ_FLOATS); b->h_rtz.resize((size_t)R * 8);
  HIPCHK(b->bounce.d2h(b->h_lin.data(), b->d_lin, R, s));
  HIPCHK(b->bounce.d2h(b->h_linAct.data(), b->Rs.active, R, s));
  HIPCHK(b->bounce.d2h(b->h_linJ.data(), b->d_fullJ, sizeof(float) * FJ_FLOATS * R, s));
  HIPCHK(b->bounce.d2h(b->h_rtz.data(), b->d_rtz, sizeof(float) * 8 * R, s));
  HIPCHK(b->bounce.finish(s));
  b->n_lin = 0;
  for (int ri = 0; ri < R; ri++) if (b->h_lin[ri]) b->n_lin++;
  b->n_lin_global = b->n_lin;
  if (sharded(b)) {   // collective: every rank of the window calls this (with the flags of its own residuals); the ranks' counts are summed
    double cnt = (double)b->n_lin;
    if (!b->d_red1) { if (dalloc(b, &b->d_red1, 1)) return -1; }
    HIPCHK(b->bounce.h2d(b->d_red1, &cnt, sizeof(double), s));
    if (int r = commAllReduceSum(b, b->d_red1, 1)) return r;
    HIPCHK(b->bounce.d2h(&cnt, b->d_red1, sizeof(double), s));
    HIPCHK(b->bounce.finish(s));
    b->n_lin_global = (long long)(cnt + 0.5);
  }
  if (linAny(b)) { b->Rs.lin = b->d_lin; b->P.lHdd = b->d_lHdd; b->P.lbd = b->d_lbd; b->P.lHcd = b->d_lHcd; b->P.HcdAF = b->d_HcdAF; }
  if (n_linearized) *n_linearized = b->n_lin;
  return 0;
}
// residuals that arrive linearised: flags (R), J74 (R x 74) and res_toZeroF (R x 8) indexed by residual; only the flagged rows travel
static int linImport(dmvio_hip_ba* b, const unsigned char* flags, const float* J74, const float* rtz, int* n_linearized) {
  const int R = b->H.R;
  hipStream_t s = b->stream;
  std::vector<int> idx;
  for (int ri = 0; ri < R; ri++) if (flags[ri]) idx.push_back(ri);
  if (idx.empty() && !sharded(b)) { if (n_linearized) *n_linearized = b->n_lin; return 0; }
  if (int r = linAlloc(b)) return r;
  const int n = (int)idx.size();
  if (n > 0) {
    std::vector<float> packed((size_t)n * FJ_PACKED);
    for (int k = 0; k < n; k++) {
      memcpy(&packed[(size_t)k * FJ_PACKED], J74 + (size_t)idx[k] * FJ_FLOATS, sizeof(float) * FJ_FLOATS);
      memcpy(&packed[(size_t)k * FJ_PACKED + FJ_FLOATS], rtz + (size_t)idx[k] * 8, sizeof(float) * 8);
    }
    int* d_idx = nullptr; float* d_packed = nullptr;
    if (dalloc(b, &d_idx, n) || dalloc(b, &d_packed, (size_t)n * FJ_PACKED)) return -1;
    HIPCHK(b->bounce.h2d(d_idx, idx.data(), sizeof(int) * n, s));
    HIPCHK(b->bounce.h2d(d_packed, packed.data(), sizeof(float) * packed.size(), s));
    hipLaunchKernelGGL(k_ba_lin_import, dim3((n + 255) / 256), dim3(256), 0, s, n, (const int*)d_idx, (const float*)d_packed, b->Rs, b->d_fullJ, b->d_rtz, b->d_linRec, b->d_lin);
    HIPCHK(hipGetLastError());
  }
  b->stateChanged();
  return linFinish(b, n_linearized);
}
// dmvio_hip_ba_set_graph from a resident graph (capi_graph.hip): the mirror flattened in makeIDX order — compact records, a few tens of microseconds — instead of arrays
// the caller rebuilt from its pointer graph.  The window (dmvio_hip_ba_set_window) must have as many keyframes as the graph.  The scratch arrays stay with the handle.
static int setGraphFrom(dmvio_hip_ba* b, dmvio_hip_graph* g) {
  int N = 0, R = 0;
  unsigned long long flat_version = 0;
  {
    std::lock_guard<std::mutex> lg(g->mu);
    if ((int)g->frames.size() != b->H.F) return failmsg("ba_set_graph_from: the graph has " + std::to_string(g->frames.size()) + " keyframes, the window " + std::to_string(b->H.F));
    if (g->nDangling) return failmsg("ba_set_graph_from: " + std::to_string(g->nDangling) + " residuals still target a removed keyframe (their dropResidual has not been forwarded)");
    N = g->nPoints; R = g->nRes;
    if (N < 1 || R < 1) return failmsg("ba_set_graph: empty graph");
    flat_version = g->version;
    auto& S = b->gscratch;
    S.host.resize(N); S.u.resize(N); S.v.resize(N); S.idepth.resize(N); S.color.resize(8 * (size_t)N); S.weights.resize(8 * (size_t)N); S.prior.resize(N);
    S.res_point.resize(R); S.res_target.resize(R);
    const bool anyLin = g->nLin > 0;   // residuals that arrive linearised: their flags / Jacobians / res_toZeroF in flat order (only then)
    if (anyLin) { S.lin.assign(R, 0); S.linJ.resize((size_t)R * FJ_FLOATS); S.linRtz.resize((size_t)R * 8); } else S.lin.clear();
    int pi = 0, ri = 0;
    for (int f = 0; f < (int)g->frames.size(); f++)
      for (const DmvGraphPoint& P : g->frames[f]) {
        S.host[pi] = f; S.u[pi] = P.u; S.v[pi] = P.v; S.idepth[pi] = P.idepth; S.prior[pi] = P.prior;
        memcpy(&S.color[8 * (size_t)pi], P.color, sizeof(P.color)); memcpy(&S.weights[8 * (size_t)pi], P.weights, sizeof(P.weights));
        for (int k = 0; k < P.nres; k++, ri++) {
          S.res_point[ri] = pi; S.res_target[ri] = P.target[k];
          if (anyLin && P.lin[k] >= 0) {
            S.lin[ri] = 1;
            memcpy(&S.linJ[(size_t)ri * FJ_FLOATS], g->linPool[P.lin[k]].J, sizeof(float) * FJ_FLOATS); memcpy(&S.linRtz[(size_t)ri * 8], g->linPool[P.lin[k]].res_toZeroF, sizeof(float) * 8);
          }
        }
        pi++;
      }
  }
  const auto& S = b->gscratch;
  if (int r = setGraphImpl(b, N, S.host.data(), S.u.data(), S.v.data(), S.idepth.data(), S.color.data(), S.weights.data(), S.prior.data(), R, S.res_point.data(), S.res_target.data(), false)) return r;
  if (!S.lin.empty()) { if (int r = linImport(b, S.lin.data(), S.linJ.data(), S.linRtz.data(), nullptr)) { b->graph_ready = false; return r; } }
  // only a window that WAS built makes its flat order the one dmvio_hip_graph_set_idepths accepts values in (until the structure changes).  The uploads are stream-ordered:
  // an asynchronous copy error of this call is reported by the next BA call that synchronises
  std::lock_guard<std::mutex> lg(g->mu);
  g->flat_version = flat_version;
  return 0;
}
