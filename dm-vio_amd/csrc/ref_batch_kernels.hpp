// Reference templates of W coarse trackers of one context per launch (dmvio_hip_tracker_set_ref_batch): the stages of ref_kernels.hpp with the window taken from
// blockIdx.y (the scheme of activate_batch_kernels.hpp).  Every kernel here calls the body its single-window form calls (refScatterBody, refPoolBody, refDilateBody,
// refCountBody, refScanBody, refWriteBody) on the planes of ONE tracker, so a tracker of a batch holds the bytes its own dmvio_hip_tracker_set_ref would have left.
//   k_ref_clear_w                                   <- the memsets of idepth[0] / weightSums[0]      (src/dso/FullSystem/CoarseTracker.cpp:141-142) and of the flow-sample mask
//   k_ref_scatter_w                                 <- the point loop                                (CoarseTracker.cpp:144-161)
//   k_ref_pool_w, k_ref_dilate_w                    <- the pyramid sums and the dilation             (CoarseTracker.cpp:164-245)
//   k_ref_count_w, k_ref_scan_w, k_ref_write_w      <- normalisation and ordered compaction          (CoarseTracker.cpp:249-293)
// A call builds one slab in pinned memory — W RefWin records, then the u, v, idepth, hdiF arrays of every window, then their per-pixel rank bytes — and uploads it in one
// copy; every kernel is handed the slab.  Nothing is shared between the windows of a launch: a workgroup touches the planes of its own window only.  The geometry
// (RefLevels) is the context's and stays a kernel argument; its `order` member is not read here — the storage order is the tracker's and comes from the record.
#pragma once
#include "ref_kernels.hpp"

namespace dmv {

struct RefWin {
  float *idp, *wsp, *idp2, *wsp2, *dense;     // the tracker's own planes (all levels back to back)
  int *tile_count, *tile_base, *seg, *pc_n;   // its block counts / bases, its (row, segment) table and its device copy of pc_n
  float4* const* pc;                          // its table of template lists
  unsigned long long* flow_mask;
  int* pc_n_row;                              // this window's row of the batch's [W][levels] table (one download per call)
  unsigned long long pts_off;                 // floats from the slab's start: u[n], v[n], idepth[n], hdiF[n]
  unsigned long long rank_off;                // bytes from the slab's start: rank[n] (read only when max_rank >= 2)
  int ref_slot, n, order, max_rank;           // max_rank: the largest per-pixel rank of this window's points
};

// A pointer read from a record in memory is a generic pointer to the compiler and every access through it a flat_* instruction (ba_batch_kernels.hpp: gl()); read through an
// lvalue whose pointee type carries the global address space it stays a global one.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wincompatible-pointer-types-discards-qualifiers"
template <class T> __device__ __forceinline__ T* refGl(T* const& member) {
  return (T*)(*reinterpret_cast<__attribute__((address_space(1))) T* const*>(&member));
}
#pragma clang diagnostic pop

// level 0 of idp / wsp and the flow mask of every window: one thread per four pixels (the planes start on an allocation boundary), the tail pixel by pixel; the mask has
// one word per 64 pixels, so the first threads of the same grid clear it
// (`third`, NULL in the host-array call: one more level-0 plane — the per-pixel counts of the from-BA call)
__device__ __forceinline__ void refClearBody(float* __restrict__ idp, float* __restrict__ wsp, float* __restrict__ third, unsigned long long* __restrict__ mask, const int n0,
                                             const int flow_words) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = 4 * t;
  if (i + 3 < n0) {
    reinterpret_cast<float4*>(idp)[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    reinterpret_cast<float4*>(wsp)[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (third) reinterpret_cast<float4*>(third)[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (int k = i; k < n0; k++) { idp[k] = 0.f; wsp[k] = 0.f; if (third) third[k] = 0.f; }
  }
  if (t < flow_words) mask[t] = 0ull;
}
__global__ void __launch_bounds__(256) k_ref_clear_w(const RefWin* __restrict__ wins, const int n0, const int flow_words) {
  const RefWin& V = wins[blockIdx.y];
  refClearBody(refGl(V.idp), refGl(V.wsp), nullptr, refGl(V.flow_mask), n0, flow_words);
}

// rank_lo == 0: the first launch (ranks 0 and 1; a window without a pixel of more than two points has no rank bytes and scatters all its points).  rank_lo >= 2: the
// launch of that one rank; windows whose largest rank is below it have nothing left
__global__ void __launch_bounds__(256) k_ref_scatter_w(const RefWin* __restrict__ wins, const float* __restrict__ slab, const int w0, const int h0, const int rank_lo,
                                                        const int rank_hi) {
  const RefWin& V = wins[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * blockDim.x) >= n) return;
  const int max_rank = V.max_rank;
  if (max_rank < rank_lo) return;
  const float* p = slab + V.pts_off;
  const unsigned char* rank = max_rank >= 2 ? reinterpret_cast<const unsigned char*>(slab) + V.rank_off : nullptr;
  refScatterBody(n, p, p + n, p + 2 * (size_t)n, p + 3 * (size_t)n, refGl(V.idp), refGl(V.wsp), w0, h0, rank, rank_lo, rank_hi);
}

__global__ void __launch_bounds__(256) k_ref_pool_w(const RefWin* __restrict__ wins, const RefLevels R) {
  const RefWin& V = wins[blockIdx.y];
  refPoolBody(R, refGl(V.idp), refGl(V.wsp));
}

__global__ void __launch_bounds__(256) k_ref_dilate_w(const RefWin* __restrict__ wins, const RefLevels R) {
  const RefWin& V = wins[blockIdx.y];
  refDilateBody(R, (const float*)refGl(V.idp), (const float*)refGl(V.wsp), refGl(V.idp2), refGl(V.wsp2));
}

__global__ void __launch_bounds__(256) k_ref_count_w(const RefWin* __restrict__ wins, const RefLevels R, const FrameStore fs) {
  const RefWin& V = wins[blockIdx.y];
  refCountBody(R, (const float*)refGl(V.idp2), (const float*)refGl(V.wsp2), fs, V.ref_slot, refGl(V.tile_count), refGl(V.seg));
}

// 2 * levels workgroups per window, as k_ref_scan; pc_n goes into the tracker's own device copy and into the window's row of the batch's table
__global__ void __launch_bounds__(1024) k_ref_scan_w(const RefWin* __restrict__ wins, const RefLevels R) {
  const RefWin& V = wins[blockIdx.y];
  refScanBody(R, (const int*)refGl(V.tile_count), refGl(V.tile_base), refGl(V.pc_n), refGl(V.seg), refGl(V.pc_n_row));
}

__global__ void __launch_bounds__(256) k_ref_write_w(const RefWin* __restrict__ wins, const RefLevels R, const FrameStore fs) {
  const RefWin& V = wins[blockIdx.y];
  refWriteBody<true>(R, V.order, (const float*)refGl(V.idp2), (const float*)refGl(V.wsp2), fs, V.ref_slot, (const int*)refGl(V.tile_base), (const int*)refGl(V.seg),
                     refGl(V.pc), refGl(V.dense), refGl(V.flow_mask));
}

// ---- dmvio_hip_tracker_set_ref_from_ba_batch: the scatter of every window out of its own resident BA window (ref_kernels.hpp: refBaCountBody / refBaScatterBody /
// refBaCrowdedBody).  A second record per window, behind the W RefWin records in the slab; the stages from k_ref_pool_w on run on the RefWin records unchanged.
//   k_ref_ba_clear_w                                 <- k_ref_clear_w, plus the count plane (level 0 of idp2) and the window's two counters
//   k_ref_ba_count_w, k_ref_ba_scatter_w, k_ref_ba_crowded_w <- the point loop (CoarseTracker.cpp:144-161) over the window's residuals; grid.x covers the largest window
struct RefBaWin {
  const int *res_point, *res_target;
  const unsigned char *newState, *active;
  const float *center, *HdiF;
  int* n_selected;     // this window's entry of the batch's table (one download per call)
  int* n_crowded;      // the tracker's own counter
  int2* crowded;       // the tracker's crowded list, `cap` entries
  int R, newest, cap, pad;
};

__global__ void __launch_bounds__(256) k_ref_ba_clear_w(const RefWin* __restrict__ wins, const RefBaWin* __restrict__ bas, const int n0, const int flow_words) {
  const RefWin& V = wins[blockIdx.y];
  const RefBaWin& S = bas[blockIdx.y];
  refClearBody(refGl(V.idp), refGl(V.wsp), refGl(V.idp2), refGl(V.flow_mask), n0, flow_words);
  if (blockIdx.x == 0 && threadIdx.x == 0) { *refGl(S.n_selected) = 0; *refGl(S.n_crowded) = 0; }
}

__global__ void __launch_bounds__(256) k_ref_ba_count_w(const RefWin* __restrict__ wins, const RefBaWin* __restrict__ bas, const int w0, const int h0) {
  const RefWin& V = wins[blockIdx.y];
  const RefBaWin& S = bas[blockIdx.y];
  const int R = S.R;
  if ((int)(blockIdx.x * blockDim.x) >= R) return;
  refBaCountBody(R, S.newest, refGl(S.res_target), refGl(S.active), refGl(S.newState), refGl(S.center), w0, h0, reinterpret_cast<int*>(refGl(V.idp2)),
                 refGl(S.n_selected));
}

__global__ void __launch_bounds__(256) k_ref_ba_scatter_w(const RefWin* __restrict__ wins, const RefBaWin* __restrict__ bas, const int w0, const int h0) {
  const RefWin& V = wins[blockIdx.y];
  const RefBaWin& S = bas[blockIdx.y];
  const int R = S.R;
  if ((int)(blockIdx.x * blockDim.x) >= R) return;
  refBaScatterBody(R, S.newest, refGl(S.res_point), refGl(S.res_target), refGl(S.active), refGl(S.newState), refGl(S.center), refGl(S.HdiF), refGl(V.idp), refGl(V.wsp),
                   w0, h0, (const int*)reinterpret_cast<int*>(refGl(V.idp2)), refGl(S.n_crowded), refGl(S.crowded), S.cap);
}

__global__ void __launch_bounds__(256) k_ref_ba_crowded_w(const RefWin* __restrict__ wins, const RefBaWin* __restrict__ bas) {
  const RefWin& V = wins[blockIdx.y];
  const RefBaWin& S = bas[blockIdx.y];
  if ((int)(blockIdx.x * blockDim.x) >= S.R) return;
  refBaCrowdedBody(refGl(S.res_point), refGl(S.center), refGl(S.HdiF), refGl(V.idp), refGl(V.wsp), (const int*)refGl(S.n_crowded), (const int2*)refGl(S.crowded), S.cap);
}

}  // namespace dmv
