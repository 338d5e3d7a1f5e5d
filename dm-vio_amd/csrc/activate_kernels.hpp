// Point activation on the device: the distance map of the active points in the newest keyframe and the choice of the immature points that become active.
//   k_dm_seed, k_dm_grow      <- CoarseDistanceMap::makeDistanceMap + growDistBFS   (src/dso/FullSystem/CoarseTracker.cpp:931-1073)
//   k_dm_add                  <- CoarseDistanceMap::addIntoDistFinal                (CoarseTracker.cpp:1076-1082)
//   k_act_classify, k_act_walk <- the candidate loop of FullSystem::activatePointsMT (src/dso/FullSystem/FullSystem.cpp:646-717)
//   k_act_gather, k_act_mark_results <- its result loop                                     (FullSystem.cpp:732-756)
//   k_rm_plan, k_rm_apply     <- its compaction, per-host swap-with-back             (FullSystem.cpp:759-770)
// The map is one byte per level-1 pixel: 0..39 = the reference's float value, DM_FAR = its 1000.  All results are integers or copies of floats: equal to the reference.
//
// growDistBFS is level-synchronous: the SET of pixels that receive k at step k does not depend on the order inside the frontier.
//   * From the 1000-filled map (makeDistanceMap) every pixel that holds k-1 was written at step k-1 and is therefore in the frontier of step k, so a step is a pull:
//     a pixel > k becomes k if a neighbour of the step's neighbourhood holds exactly k-1 and does not lie on the image border (border pixels do not expand,
//     :995 / :1026).  In place: the only value written during step k is k, to pixels that held more, and neither is k-1.
//   * From one seed on a map that already holds values (addIntoDistFinal) old pixels holding k-1 are NOT frontier: the frontier is an explicit list.  A frontier
//     entry claims a neighbour with a compare-and-swap on the map word that holds the neighbour's byte, so every pixel enters the next list once, as in the
//     reference's sequential `> k` test.  The lists hold at most the ring of the step (< 8 * 39 pixels).
// The candidate loop is greedy, but the map only ever decreases while it runs: a candidate that fails `dist >= minActDist * my_type` on the map makeDistanceMap
// left fails at any later time.  k_act_classify does everything that is independent per point (deletions, canActivate, projection, that prefilter); k_act_walk,
// ONE workgroup, puts the survivors into the reference's order and walks them: up to blockDim survivors are tested against the current map at once, the first
// that passes is accepted (all before it have failed on the very map the reference would have tested them on), its BFS is grown, the walk resumes behind it.
// The map lives in LDS for the walk (ACT_LDS: 160 KiB per workgroup on gfx950) or stays in global memory (L2-resident) when it does not fit.
#pragma once
#include "common.h"
#include "immature_types.hpp"

namespace dmv {

enum { DM_FAR = 255, DM_STEPS = 40, ACT_THREADS = 1024, ACT_LIST = 1024, ACT_LDS_BUDGET = 160 * 1024 };
enum { ACTC_CLASSIFIED = 0, ACTC_SURVIVORS, ACTC_ACCEPTED, ACTC_DELETED, ACTC_NEW_N, ACTC_ACTIVATED, ACTC_TAGS = 8 };
// dynamic LDS of k_act_walk / k_dm_add: [map bytes (LDS variant only, padded to 16) | two frontier lists]
extern __shared__ __attribute__((aligned(16))) unsigned char s_act_dyn[];

struct DmGeom { int w1, h1; };

__device__ __forceinline__ float dmValue(const unsigned int b) { return b == DM_FAR ? 1000.f : (float)b; }

// Vec3f ptp = KRKi * Vec3f(u, v, 1) + Kt * idepth; int(ptp[0] / ptp[2] + 0.5f): the product order of k_immature_trace (immature_kernels.hpp), no contraction
__device__ __forceinline__ bool dmProject(const float* __restrict__ KRKi, const float* __restrict__ Kt, const float u, const float v, const float idepth, const DmGeom G,
                                          int* pix, float* ptp0) {
  const float pr0 = KRKi[0] * u + KRKi[1] * v + KRKi[2] * 1.0f, pr1 = KRKi[3] * u + KRKi[4] * v + KRKi[5] * 1.0f, pr2 = KRKi[6] * u + KRKi[7] * v + KRKi[8] * 1.0f;
  const float p0 = pr0 + Kt[0] * idepth, p1 = pr1 + Kt[1] * idepth, p2 = pr2 + Kt[2] * idepth;
  const float fu = p0 / p2 + 0.5f, fv = p1 / p2 + 0.5f;
  // the reference's float -> int conversion yields INT_MIN for NaN and for values outside int; every such value fails the window test, as here
  if (!(fu > -2147483648.f && fu < 2147483648.f && fv > -2147483648.f && fv < 2147483648.f)) return false;
  const int iu = (int)fu, iv = (int)fv;
  if (!(iu > 0 && iv > 0 && iu < G.w1 && iv < G.h1)) return false;
  *pix = iu + G.w1 * iv;
  *ptp0 = p0;
  return true;
}

// makeDistanceMap's seeds (:945-964): every active point projected with its host's row; the map was filled with DM_FAR before
__device__ __forceinline__ void dmSeedBody(const int n, const int* __restrict__ host, const float* __restrict__ u, const float* __restrict__ v,
                                                  const float* __restrict__ idepth, const float* __restrict__ KRKi, const float* __restrict__ Kt, const DmGeom G,
                                                  unsigned char* __restrict__ map) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int hI = host[i];
  int pix; float p0;
  if (dmProject(KRKi + 9 * hI, Kt + 3 * hI, u[i], v[i], idepth[i], G, &pix, &p0)) map[pix] = 0;
}
__global__ void __launch_bounds__(256) k_dm_seed(const int n, const int* __restrict__ host, const float* __restrict__ u, const float* __restrict__ v,
                                                  const float* __restrict__ idepth, const float* __restrict__ KRKi, const float* __restrict__ Kt, const DmGeom G,
                                                  unsigned char* __restrict__ map) {
  dmSeedBody(n, host, u, v, idepth, KRKi, Kt, G, map);
}

// one step of growDistBFS from the freshly seeded map, as a pull (see above); k odd: 8-neighbourhood, k even: 4-neighbourhood
__device__ __forceinline__ void dmGrowBody(unsigned char* map, const DmGeom G, const int k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G.w1 * G.h1) return;
  if ((int)map[i] <= k) return;
  const int x = i % G.w1, y = i / G.w1;
  const int want = k - 1;
  bool hit = false;
#pragma unroll
  for (int d = 0; d < 8; d++) {
    const int dx = d == 0 ? 1 : d == 1 ? -1 : d < 4 ? 0 : ((d == 4 || d == 7) ? 1 : -1);
    const int dy = d < 2 ? 0 : d == 2 ? 1 : d == 3 ? -1 : (d < 6 ? 1 : -1);
    if (d >= 4 && !(k & 1)) continue;
    const int qx = x + dx, qy = y + dy;
    // the neighbour must be an interior pixel: a frontier pixel on the border does not expand
    if (qx < 1 || qy < 1 || qx >= G.w1 - 1 || qy >= G.h1 - 1) continue;
    if ((int)map[qx + qy * G.w1] == want) hit = true;
  }
  if (hit) map[i] = (unsigned char)k;
}
__global__ void __launch_bounds__(256) k_dm_grow(unsigned char* map, const DmGeom G, const int k) { dmGrowBody(map, G, k); }

// ------------------------------------------------------------------------------------------------------------------------
// the map as the single-workgroup kernels see it: LDS (s_act_dyn) or global memory
template <bool LDS> struct ActMap {
  unsigned char* g;
  __device__ __forceinline__ unsigned int ld(const int i) const {
    if constexpr (LDS) return s_act_dyn[i];
    else return __hip_atomic_load(g + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // past the CU's vector cache: the claims below are made in L2
  }
  __device__ __forceinline__ void st(const int i, const unsigned int v) const {
    if constexpr (LDS) s_act_dyn[i] = (unsigned char)v;
    else __hip_atomic_store(g + i, (unsigned char)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // pixel q takes value k if it holds more; true for the one caller that changed it
  __device__ __forceinline__ bool claim(const int q, const int k) const {
    unsigned int* wp;
    if constexpr (LDS) wp = reinterpret_cast<unsigned int*>(s_act_dyn) + (q >> 2);
    else wp = reinterpret_cast<unsigned int*>(g) + (q >> 2);
    const int sh = (q & 3) * 8;
    unsigned int old;
    if constexpr (LDS) old = __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else old = __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
      if (((old >> sh) & 255u) <= (unsigned int)k) return false;
      const unsigned int nw = (old & ~(255u << sh)) | ((unsigned int)k << sh);
      const unsigned int prev = atomicCAS(wp, old, nw);
      if (prev == old) return true;
      old = prev;
    }
  }
};

// addIntoDistFinal(u, v) by the whole workgroup: seed 0, then growDistBFS(1) with an explicit frontier and early exit once it is empty.  lists: 2 x ACT_LIST packed
// pixels (x | y << 16) in LDS; s_cnt[k] = length of the frontier step k reads.  Every thread of the workgroup calls it with the same seed.
template <bool LDS>
__device__ __forceinline__ void actGrowFrom(const ActMap<LDS> M, int* __restrict__ lists, int* __restrict__ s_cnt, const DmGeom G, const int su, const int sv) {
  const int tid = threadIdx.x;
  __syncthreads();   // the callers' reads of the map and of s_cnt are done
  if (tid <= DM_STEPS) s_cnt[tid] = tid == 1 ? 1 : 0;
  if (tid == 0) { M.st(su + G.w1 * sv, 0); lists[ACT_LIST] = su | (sv << 16); }   // step 1 reads list 1
  __syncthreads();
  for (int k = 1; k < DM_STEPS; k++) {
    const int n = min(s_cnt[k], (int)ACT_LIST);
    if (n == 0) break;
    const int* cur = lists + (k & 1) * ACT_LIST;
    int* nxt = lists + ((k + 1) & 1) * ACT_LIST;
    const int ndir = (k & 1) ? 8 : 4;
    for (int item = tid; item < n * 8; item += blockDim.x) {
      const int d = item & 7;
      if (d >= ndir) continue;
      const int p = cur[item >> 3];
      const int x = p & 0xffff, y = p >> 16;
      if (x == 0 || y == 0 || x == G.w1 - 1 || y == G.h1 - 1) continue;
      const int dx = d == 0 ? 1 : d == 1 ? -1 : d < 4 ? 0 : ((d == 4 || d == 7) ? 1 : -1);
      const int dy = d < 2 ? 0 : d == 2 ? 1 : d == 3 ? -1 : (d < 6 ? 1 : -1);
      const int qx = x + dx, qy = y + dy;
      if (M.claim(qx + qy * G.w1, k)) {
        const int pos = atomicAdd(&s_cnt[k + 1], 1);
        if (pos < ACT_LIST) nxt[pos] = qx | (qy << 16);
      }
    }
    __syncthreads();
  }
  __syncthreads();
}

// dmvio_hip_distance_map_add: one addIntoDistFinal on the map in global memory
__global__ void __launch_bounds__(ACT_THREADS) k_dm_add(unsigned char* map, const DmGeom G, const int u, const int v) {
  __shared__ int s_cnt[DM_STEPS + 2];
  ActMap<false> M; M.g = map;
  actGrowFrom<false>(M, reinterpret_cast<int*>(s_act_dyn), s_cnt, G, u, v);
}

// ------------------------------------------------------------------------------------------------------------------------
struct ActArgs {
  int n, n_hosts, newest_tag;
  float minActDist, minTraceQuality;
  const float *KRKi, *Kt;          // device tables, n_hosts rows
  const unsigned char* flagged;    // n_hosts bytes: FrameHessian::flaggedForMarginalization
};

// FullSystem.cpp:655-716 without the order-dependent part: decision 2 = deleted, 0 = stays, 3 = passed `dist >= minActDist * my_type` on the initial map
__device__ __forceinline__ void actClassifyBody(const ImmaturePts P, const ActArgs A, const DmGeom G, const unsigned char* __restrict__ map, int* __restrict__ decision,
                                                       int* __restrict__ pidx, float* __restrict__ frac, float* __restrict__ thr, int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const int hI = P.host[i];
  int dec = 0;
  if (hI != A.newest_tag) {
    const float imax = P.idepth_max[i], imin = P.idepth_min[i];
    const int status = P.lastTraceStatus[i];
    if (!isfinite(imax) || status == IPS_OUTLIER) dec = 2;
    else {
      const bool canActivate = (status == IPS_GOOD || status == IPS_SKIPPED || status == IPS_BADCONDITION || status == IPS_OOB) && P.lastTracePixelInterval[i] < 8 &&
                               P.quality[i] > A.minTraceQuality && (imax + imin) > 0;
      if (!canActivate) dec = (A.flagged[hI] || status == IPS_OOB) ? 2 : 0;
      else {
        int pix; float p0;
        if (!dmProject(A.KRKi + 9 * hI, A.Kt + 3 * hI, P.u[i], P.v[i], 0.5f * (imax + imin), G, &pix, &p0)) dec = 2;
        else {
          const float f = p0 - floorf(p0), t = A.minActDist * P.my_type[i];
          pidx[i] = pix; frac[i] = f; thr[i] = t;
          atomicAdd(&counts[ACTC_CLASSIFIED], 1);
          if (dmValue(map[pix]) + f >= t) { dec = 3; atomicAdd(&counts[ACTC_SURVIVORS], 1); }
        }
      }
    }
    if (dec == 2) atomicAdd(&counts[ACTC_DELETED], 1);
  }
  decision[i] = dec;
}
__global__ void __launch_bounds__(256) k_act_classify(const ImmaturePts P, const ActArgs A, const DmGeom G, const unsigned char* __restrict__ map, int* __restrict__ decision,
                                                       int* __restrict__ pidx, float* __restrict__ frac, float* __restrict__ thr, int* __restrict__ counts) {
  actClassifyBody(P, A, G, map, decision, pidx, frac, thr, counts);
}

// exclusive rank of `flag` among the workgroup's threads (thread order) + the workgroup's total; s_w: one int per wave.  Two barriers.
__device__ __forceinline__ int actBlockRank(const bool flag, int* __restrict__ s_w, int* total) {
  const unsigned long long b = __ballot(flag);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();   // s_w of a previous call has been read
  if (lane == 0) s_w[wv] = __popcll(b);
  __syncthreads();
  int pre = 0, all = 0;
  for (int k = 0; k < nw; k++) { const int s = s_w[k]; if (k < wv) pre += s; all += s; }
  *total = all;
  return pre + before;
}

// the ordered walk (see the head of this file).  One workgroup.  The final map is written back (LDS variant) / is the global map itself.
template <bool LDS>
__device__ __forceinline__ void actWalkBody(const ImmaturePts P, const ActArgs A, const DmGeom G, unsigned char* gmap, const int map_bytes /* multiple of 16 */,
                                                           int* __restrict__ decision, const int* __restrict__ pidx, const float* __restrict__ frac,
                                                           const float* __restrict__ thr, int* surv, int* __restrict__ order, unsigned char* __restrict__ select,
                                                           unsigned char* __restrict__ mark, int* __restrict__ counts) {
  __shared__ int s_cnt[DM_STEPS + 2];
  __shared__ int s_w[ACT_THREADS / 64];
  __shared__ int s_first;
  const int tid = threadIdx.x;
  ActMap<LDS> M; M.g = gmap;
  int* lists = reinterpret_cast<int*>(s_act_dyn + (LDS ? map_bytes : 0));
  if constexpr (LDS) {
    const uint4* src = reinterpret_cast<const uint4*>(gmap);
    uint4* dst = reinterpret_cast<uint4*>(s_act_dyn);
    for (int i = tid; i < map_bytes / 16; i += blockDim.x) dst[i] = src[i];
  }
  // 1. the reference's order: hosts by ascending tag (the newest has no survivors), points of a host by ascending index
  int ns = 0;
  for (int t = 0; t < A.n_hosts; t++) {
    if (t == A.newest_tag) continue;
    for (int base = 0; base < A.n; base += blockDim.x) {
      const int i = base + tid;
      const bool f = i < A.n && decision[i] == 3 && P.host[i] == t;
      int total;
      const int r = actBlockRank(f, s_w, &total);
      if (f) surv[ns + r] = i;
      ns += total;
    }
  }
  __syncthreads();   // surv (global, written by this workgroup) and the LDS map are complete
  // 2. the walk
  int cursor = 0, nacc = 0;
  while (cursor < ns) {
    if (tid == 0) s_first = 0x7fffffff;
    __syncthreads();
    const int j = cursor + tid;
    bool pass = false;
    if (j < ns) {
      const int s = surv[j];
      pass = dmValue(M.ld(pidx[s])) + frac[s] >= thr[s];
    }
    const unsigned long long b = __ballot(pass);
    if (b != 0ull && (tid & 63) == 0) atomicMin(&s_first, tid + __ffsll((unsigned long long)b) - 1);
    __syncthreads();
    const int first = s_first;
    __syncthreads();   // everyone has read s_first before the next round resets it
    if (first == 0x7fffffff) { cursor += blockDim.x; continue; }   // all of them rejected on the current map
    const int s = surv[cursor + first];
    if (tid == 0) { decision[s] = 1; order[nacc] = s; }
    nacc++;
    const int pix = pidx[s];
    actGrowFrom<LDS>(M, lists, s_cnt, G, pix % G.w1, pix / G.w1);
    cursor += first + 1;
  }
  __syncthreads();
  // 3. results: survivors that were not accepted stay; the masks of the later steps; the map
  for (int i = tid; i < A.n; i += blockDim.x) {
    int d = decision[i];
    if (d == 3) { d = 0; decision[i] = 0; }
    select[i] = d == 1;
    mark[i] = d == 2;
  }
  if constexpr (LDS) {
    uint4* dst = reinterpret_cast<uint4*>(gmap);
    const uint4* src = reinterpret_cast<const uint4*>(s_act_dyn);
    for (int i = tid; i < map_bytes / 16; i += blockDim.x) dst[i] = src[i];
  }
  if (tid == 0) counts[ACTC_ACCEPTED] = nacc;
}
template <bool LDS>
__global__ void __launch_bounds__(ACT_THREADS) k_act_walk(const ImmaturePts P, const ActArgs A, const DmGeom G, unsigned char* gmap, const int map_bytes /* multiple of 16 */,
                                                           int* __restrict__ decision, const int* __restrict__ pidx, const float* __restrict__ frac,
                                                           const float* __restrict__ thr, int* surv, int* __restrict__ order, unsigned char* __restrict__ select,
                                                           unsigned char* __restrict__ mark, int* __restrict__ counts) {
  actWalkBody<LDS>(P, A, G, gmap, map_bytes, decision, pidx, frac, thr, surv, order, select, mark, counts);
}

// FullSystem.cpp:732-756 for the optimised selection, in toOptimize order: the results gathered, the deletion marks (activated points leave the immature list, failed
// ones and not-converged OOB ones are deleted), and the record the PointHessian constructor copies (HessianBlocks.cpp:36-58)
__device__ __forceinline__ void actGatherBody(const ImmaturePts P, const int n_sel, const int F, const int* __restrict__ order, const int* __restrict__ result,
                                                     const float* __restrict__ idepth, const int* __restrict__ res_state, unsigned char* __restrict__ mark,
                                                     int* __restrict__ gi, float* __restrict__ gf, int* __restrict__ counts) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_sel) return;
  const int i = order[k];
  const int res = result[i];
  gi[k] = res;
  gi[n_sel + k] = P.host[i];
  for (int t = 0; t < 8; t++) gi[2 * n_sel + 8 * k + t] = t < F ? res_state[(size_t)i * F + t] : -1;
  gf[k] = idepth[i];
  gf[1 * n_sel + k] = P.u[i]; gf[2 * n_sel + k] = P.v[i]; gf[3 * n_sel + k] = P.my_type[i];
  gf[4 * n_sel + k] = P.idepth_min[i]; gf[5 * n_sel + k] = P.idepth_max[i]; gf[6 * n_sel + k] = P.energyTH[i];
  for (int t = 0; t < 8; t++) { gf[7 * n_sel + 8 * k + t] = P.color[8 * i + t]; gf[15 * n_sel + 8 * k + t] = P.weights[8 * i + t]; }
  if (res == 1 || res == -1 || (res == 0 && P.lastTraceStatus[i] == IPS_OOB)) mark[i] = 1;
  if (res == 1) atomicAdd(&counts[ACTC_ACTIVATED], 1);
}
__global__ void __launch_bounds__(256) k_act_gather(const ImmaturePts P, const int n_sel, const int F, const int* __restrict__ order, const int* __restrict__ result,
                                                     const float* __restrict__ idepth, const int* __restrict__ res_state, unsigned char* __restrict__ mark,
                                                     int* __restrict__ gi, float* __restrict__ gf, int* __restrict__ counts) {
  actGatherBody(P, n_sel, F, order, result, idepth, res_state, mark, gi, gf, counts);
}

// the marks of FullSystem.cpp:732-756 from results computed elsewhere (result[k] of toOptimize[k])
__global__ void __launch_bounds__(256) k_act_mark_results(const ImmaturePts P, const int n_sel, const int* __restrict__ order, const int* __restrict__ result,
                                                           unsigned char* __restrict__ mark) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_sel) return;
  const int i = order[k], res = result[k];
  if (res == 1 || res == -1 || (res == 0 && P.lastTraceStatus[i] == IPS_OOB)) mark[i] = 1;
}

__global__ void __launch_bounds__(256) k_rm_mark_host(const ImmaturePts P, const int n, const int tag, unsigned char* __restrict__ mark) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mark[i] = P.host[i] == tag;
}

// The reference compacts every host's list with `list[i] = list.back(); pop_back(); i--` (FullSystem.cpp:759-770).  With m survivors in a list, survivors at
// positions < m stay, and the holes below m, in ascending order, receive the survivors at positions >= m in DESCENDING order.  Both ranks are scans.  One workgroup;
// hosts are packed in ascending tag.  newidx[i] = new handle index or -1; counts[ACTC_NEW_N] = new count, counts[ACTC_TAGS + t] = points of tag t afterwards.
__device__ __forceinline__ void rmPlanBody(const int* __restrict__ host, const unsigned char* __restrict__ mark, const int n, const int n_tags, int* newidx,
                                                          int* holes, int* __restrict__ counts) {
  __shared__ int s_w[ACT_THREADS / 64];
  __shared__ int s_m;
  const int tid = threadIdx.x;
  int outBase = 0;
  for (int t = 0; t < n_tags; t++) {
    if (tid == 0) s_m = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += blockDim.x) mine += (host[i] == t && !mark[i]) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if ((tid & 63) == 0 && mine) atomicAdd(&s_m, mine);
    __syncthreads();
    const int m = s_m;
    int pos0 = 0, nholes = 0, nmovers = 0;
    for (int base = 0; base < n; base += blockDim.x) {
      const int i = base + tid;
      const bool same = i < n && host[i] == t;
      int tot;
      const int pos = pos0 + actBlockRank(same, s_w, &tot);
      pos0 += tot;
      const bool del = same && mark[i];
      const bool hole = del && pos < m, mover = same && !del && pos >= m;
      const int hr = nholes + actBlockRank(hole, s_w, &tot);
      nholes += tot;
      const int mr = nmovers + actBlockRank(mover, s_w, &tot);
      nmovers += tot;
      if (hole) holes[hr] = pos;
      if (del) newidx[i] = -1;
      else if (mover) newidx[i] = -2 - mr;
      else if (same) newidx[i] = outBase + pos;
    }
    __syncthreads();   // holes (global, written by this workgroup) is complete
    for (int i = tid; i < n; i += blockDim.x) {
      if (host[i] != t) continue;
      const int v = newidx[i];
      if (v <= -2) newidx[i] = outBase + holes[nmovers - 1 - (-2 - v)];
    }
    if (tid == 0) counts[ACTC_TAGS + t] = m;
    outBase += m;
    __syncthreads();
  }
  if (tid == 0) counts[ACTC_NEW_N] = outBase;
}
__global__ void __launch_bounds__(ACT_THREADS) k_rm_plan(const int* __restrict__ host, const unsigned char* __restrict__ mark, const int n, const int n_tags, int* newidx,
                                                          int* holes, int* __restrict__ counts) {
  rmPlanBody(host, mark, n, n_tags, newidx, holes, counts);
}

// drop_tag >= 0: tags above it move down by one (a marginalised keyframe leaves the window)
__device__ __forceinline__ void rmApplyBody(const ImmaturePts S, const ImmaturePts D, const int n, const int* __restrict__ newidx, const int drop_tag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int j = newidx[i];
  if (j < 0) return;
  D.u[j] = S.u[i]; D.v[j] = S.v[i];
  const int hI = S.host[i];
  D.host[j] = (drop_tag >= 0 && hI > drop_tag) ? hI - 1 : hI;
  for (int t = 0; t < 8; t++) { D.color[8 * j + t] = S.color[8 * i + t]; D.weights[8 * j + t] = S.weights[8 * i + t]; }
  for (int t = 0; t < 4; t++) D.gradH[4 * j + t] = S.gradH[4 * i + t];
  D.energyTH[j] = S.energyTH[i]; D.idepth_min[j] = S.idepth_min[i]; D.idepth_max[j] = S.idepth_max[i]; D.quality[j] = S.quality[i];
  D.lastTraceUV[2 * j] = S.lastTraceUV[2 * i]; D.lastTraceUV[2 * j + 1] = S.lastTraceUV[2 * i + 1];
  D.lastTracePixelInterval[j] = S.lastTracePixelInterval[i]; D.lastTraceStatus[j] = S.lastTraceStatus[i]; D.my_type[j] = S.my_type[i];
}
__global__ void __launch_bounds__(256) k_rm_apply(const ImmaturePts S, const ImmaturePts D, const int n, const int* __restrict__ newidx, const int drop_tag) {
  rmApplyBody(S, D, n, newidx, drop_tag);
}

}  // namespace dmv
