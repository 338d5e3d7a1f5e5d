// Point activation for W sliding windows per launch: the kernels of activate_kernels.hpp with the window taken from the block index (the scheme of ba_batch_kernels.hpp).
// Every kernel here calls the body its single-window form calls (dmSeedBody, dmGrowBody, actClassifyBody, actWalkBody, actGatherBody, rmPlanBody, rmApplyBody) on the arrays
// of ONE window, so a window of a batch holds the bytes its single call would have left.
//   k_dm_fill_b, k_dm_seed_b, k_dm_grow_b   <- CoarseDistanceMap::makeDistanceMap + growDistBFS   (src/dso/FullSystem/CoarseTracker.cpp:931-1073)
//   k_act_classify_b, k_act_ordered_walk_b  <- the candidate loop of FullSystem::activatePointsMT (src/dso/FullSystem/FullSystem.cpp:646-717)
//   k_act_gather_b                          <- its result loop                                     (FullSystem.cpp:732-756)
//   k_rm_plan_b, k_rm_apply_b               <- its compaction                                      (FullSystem.cpp:759-770)
// A call builds one slab of ActWin records (pinned, one upload) and hands every kernel the slab.  The ordered walk stays what it is inside a window — one workgroup, sequential
// in the candidates — and the batch is W such workgroups side by side: grid = W, nothing shared between them, no workgroup waits for another.  Whatever a workgroup loops on
// (n, the survivors, the host count) comes from its own record and is the same for all its threads; a window without points, or a block past its window's size, returns
// before the first barrier as a whole.
#pragma once
#include "activate_kernels.hpp"

namespace dmv {

struct ActWin {
  ImmaturePts P, P2;               // the handle's points and the arrays its compaction writes
  ActArgs A;                       // of the select call: n, n_hosts, newest_tag, the two thresholds, tables and flags (in the call's slab)
  unsigned char* map; int map_bytes;
  int n, n_active, n_sel, F, n_tags;
  int *decision, *pidx; float *frac, *thr; int *surv, *order; unsigned char *select, *mark;
  int* counts;                     // ACTC_* of this window, 8 + 64 ints in the batch's count slab (one download per call)
  int *newidx, *holes;
  const int* result; const float* idepth; const int* res_state; int* gather_i; float* gather_f;   // optimize_selected
  const int* act_host; const float *act_u, *act_v, *act_idepth, *mk_KRKi, *mk_Kt;                  // the active points and tables of make, staged in the call's slab
};

// A pointer read from a record in memory is a generic pointer to the compiler and every access through it a flat_* instruction (ba_batch_kernels.hpp: gl()); read through an
// lvalue whose pointee type carries the global address space it stays a global one.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wincompatible-pointer-types-discards-qualifiers"
template <class T> __device__ __forceinline__ T* actGl(T* const& member) {
  return (T*)(*reinterpret_cast<__attribute__((address_space(1))) T* const*>(&member));
}
#pragma clang diagnostic pop
__device__ __forceinline__ ImmaturePts actPts(const ImmaturePts& g) {
  ImmaturePts v;
  v.n = g.n;
  v.u = actGl(g.u); v.v = actGl(g.v); v.host = actGl(g.host); v.color = actGl(g.color); v.weights = actGl(g.weights); v.gradH = actGl(g.gradH); v.energyTH = actGl(g.energyTH);
  v.idepth_min = actGl(g.idepth_min); v.idepth_max = actGl(g.idepth_max); v.quality = actGl(g.quality); v.lastTraceUV = actGl(g.lastTraceUV);
  v.lastTracePixelInterval = actGl(g.lastTracePixelInterval); v.lastTraceStatus = actGl(g.lastTraceStatus); v.my_type = actGl(g.my_type);
  return v;
}
__device__ __forceinline__ ActArgs actArgs(const ActArgs& g) {
  ActArgs v = g;
  v.KRKi = actGl(g.KRKi); v.Kt = actGl(g.Kt); v.flagged = actGl(g.flagged);
  return v;
}

// window = blockIdx.y (grid.x is the largest count of the batch) or, for the one-workgroup kernels, blockIdx.x
__global__ void __launch_bounds__(256) k_dm_fill_b(const ActWin* __restrict__ wins) {
  const ActWin& V = wins[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V.map_bytes / 16) return;
  reinterpret_cast<uint4*>(actGl(V.map))[i] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);   // DM_FAR in every byte
}
__global__ void __launch_bounds__(256) k_dm_seed_b(const ActWin* __restrict__ wins, const DmGeom G) {
  const ActWin& V = wins[blockIdx.y];
  if ((int)(blockIdx.x * blockDim.x) >= V.n_active) return;
  dmSeedBody(V.n_active, actGl(V.act_host), actGl(V.act_u), actGl(V.act_v), actGl(V.act_idepth), actGl(V.mk_KRKi), actGl(V.mk_Kt), G, actGl(V.map));
}
__global__ void __launch_bounds__(256) k_dm_grow_b(const ActWin* __restrict__ wins, const DmGeom G, const int k) {
  const ActWin& V = wins[blockIdx.y];
  if (V.n_active == 0) return;   // no seed: the map stays DM_FAR, as the single call leaves it without a launch
  dmGrowBody(actGl(V.map), G, k);
}
__global__ void __launch_bounds__(256) k_act_classify_b(const ActWin* __restrict__ wins, const DmGeom G) {
  const ActWin& V = wins[blockIdx.y];
  if ((int)(blockIdx.x * blockDim.x) >= V.n) return;
  actClassifyBody(actPts(V.P), actArgs(V.A), G, (const unsigned char*)actGl(V.map), actGl(V.decision), actGl(V.pidx), actGl(V.frac), actGl(V.thr), actGl(V.counts));
}
template <bool LDS>
__global__ void __launch_bounds__(ACT_THREADS) k_act_ordered_walk_b(const ActWin* __restrict__ wins, const DmGeom G) {
  const ActWin& V = wins[blockIdx.x];
  if (V.n == 0) return;
  actWalkBody<LDS>(actPts(V.P), actArgs(V.A), G, actGl(V.map), V.map_bytes, actGl(V.decision), (const int*)actGl(V.pidx), (const float*)actGl(V.frac),
                   (const float*)actGl(V.thr), actGl(V.surv), actGl(V.order), actGl(V.select), actGl(V.mark), actGl(V.counts));
}
__global__ void __launch_bounds__(256) k_act_gather_b(const ActWin* __restrict__ wins) {
  const ActWin& V = wins[blockIdx.y];
  if ((int)(blockIdx.x * blockDim.x) >= V.n_sel) return;
  actGatherBody(actPts(V.P), V.n_sel, V.F, (const int*)actGl(V.order), actGl(V.result), actGl(V.idepth), actGl(V.res_state), actGl(V.mark), actGl(V.gather_i),
                actGl(V.gather_f), actGl(V.counts));
}
__global__ void __launch_bounds__(ACT_THREADS) k_rm_plan_b(const ActWin* __restrict__ wins) {
  const ActWin& V = wins[blockIdx.x];
  if (V.n == 0) return;
  rmPlanBody((const int*)actGl(V.P.host), (const unsigned char*)actGl(V.mark), V.n, V.n_tags, actGl(V.newidx), actGl(V.holes), actGl(V.counts));
}
__global__ void __launch_bounds__(256) k_rm_apply_b(const ActWin* __restrict__ wins) {
  const ActWin& V = wins[blockIdx.y];
  if ((int)(blockIdx.x * blockDim.x) >= V.n) return;
  rmApplyBody(actPts(V.P), actPts(V.P2), V.n, (const int*)actGl(V.newidx), -1);
}

}  // namespace dmv
