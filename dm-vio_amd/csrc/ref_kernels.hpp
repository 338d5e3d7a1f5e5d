// Reference-template construction of the coarse tracker on the device.
// Replaces CoarseTracker::makeCoarseDepthL0 (src/dso/FullSystem/CoarseTracker.cpp:138-295):
//   scatter of weighted inverse depths (:144-161), 2x2 sum-pool down the pyramid (:164-189),
//   1-pixel dilation — diagonal neighbours on levels 0/1 (:193-220), 4-neighbourhood above (:224-245) —
//   normalisation and row-major compaction into pc_u/pc_v/pc_idepth/pc_color (:249-293).
// The compaction is an ORDERED (deterministic) stream compaction: counts -> exclusive scan -> ranked write.
// Template points are emitted in TILE order (8x8-pixel tiles, Z-ordered inside 16x16 blocks, blocks row-major) rather
// than the reference's row-major order: neighbouring lanes then tap neighbouring pixels, so the dilated 3x3 clusters
// around each active point share cache lines.  Sums do not depend on the order; the one order-dependent rule of the
// reference — flow indicators are sampled at every 32nd point of the ROW-MAJOR list (CoarseTracker.cpp:416) — is kept
// exactly: each point's row-major rank is reconstructed from per-(row, tile) counts and stored as a bit mask.
#pragma once
#include "common.h"

namespace dmv {

// The reference adds the points of a pixel one after the other (CoarseTracker.cpp:151-165).  Two float atomics on one pixel commute (0 + a + b); a third
// would make the sum depend on the arrival order, so the host ranks the points of every pixel by index (`rank`, NULL when no pixel holds more than two) and
// launches ranks [0,1] together and every further rank as its own launch behind them: sequential order, no data race.
// (every stage below is a __device__ body that its single-window kernel here and its W-window kernel in ref_batch_kernels.hpp both call: the arithmetic and its operand
// order exist once)
// the level-0 pixel a point lands on (CoarseTracker.cpp:147-148), or -1: the reference would write out of bounds there; and its weight (:149).  Each exists once: the
// scatter of host arrays below and the scatter out of a resident BA window (refBa*Body) call them
__device__ __forceinline__ int refPointPixel(const float u, const float v, const int w0, const int h0) {
  const int ui = (int)(u + 0.5f);
  const int vi = (int)(v + 0.5f);
  if (ui < 0 || vi < 0 || ui >= w0 || vi >= h0) return -1;
  return ui + w0 * vi;
}
__device__ __forceinline__ float refPointWeight(const float hdiF) { return sqrtf((float)(1e-3 / ((double)hdiF + 1e-12))); }

__device__ __forceinline__ void refScatterBody(const int n, const float* __restrict__ u, const float* __restrict__ v,
                                               const float* __restrict__ idepth, const float* __restrict__ hdiF,
                                               float* __restrict__ id0, float* __restrict__ ws0, const int w0, const int h0,
                                               const unsigned char* __restrict__ rank, const int rank_lo, const int rank_hi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (rank) { const int r = rank[i]; if (r < rank_lo || r > rank_hi) return; }
  const int pix = refPointPixel(u[i], v[i], w0, h0);
  if (pix < 0) return;
  const float weight = refPointWeight(hdiF[i]);
  atomicAdd(&id0[pix], idepth[i] * weight);
  atomicAdd(&ws0[pix], weight);
}
__global__ void __launch_bounds__(256) k_ref_scatter(const int n, const float* __restrict__ u, const float* __restrict__ v,
                                                      const float* __restrict__ idepth, const float* __restrict__ hdiF,
                                                      float* __restrict__ id0, float* __restrict__ ws0, const int w0, const int h0,
                                                      const unsigned char* __restrict__ rank, const int rank_lo, const int rank_hi) {
  refScatterBody(n, u, v, idepth, hdiF, id0, ws0, w0, h0, rank, rank_lo, rank_hi);
}

// ---- the same scatter out of a resident BA window (dmvio_hip_tracker_set_ref_from_ba): the points are the residuals to the newest keyframe that are active and IN
// (CoarseTracker.cpp:144-146: `r->efResidual->isActive() && r->target == lastRef`, state IN), read where the window optimiser left them — centerProjectedTo and the
// point's HdiF — in the graph's residual order.  The host never sees them, so it cannot rank them; the index order per pixel is kept by three launches instead:
//   (a) refBaCountBody    one thread per residual: the selected points per level-0 pixel, in an int plane (level 0 of the dilated idepth plane, which k_ref_dilate
//                         overwrites later), and the number of selected residuals
//   (b) refBaScatterBody  one thread per selected residual: a pixel of at most two points takes the two atomics (0 + a + b commutes); a point of a fuller pixel appends
//                         (pixel, residual) to the window's crowded list instead (any order)
//   (c) refBaCrowdedBody  one thread per list entry: the entry with the lowest residual index of its pixel (none lower in the list) adds that pixel's entries in
//                         ascending index order with plain adds onto the untouched pixel — the sum the rank launches of the host-array call form
// The list has room for every residual of the window (the caller sizes it), so it cannot overflow; a residual beyond `cap` would be dropped, never written.
struct RefBaSrc {
  const int *res_point, *res_target;          // BARes::point / target
  const unsigned char *newState, *active;     // BARes::newState (0 = IN) / active
  const float *center, *HdiF;                 // BARes::center (R x 3: u, v, idepth), BAPoints::HdiF
  int R, newest;                              // residuals of the graph, index of the newest keyframe
};
__device__ __forceinline__ bool refBaSelected(const int r, const int R, const int newest, const int* __restrict__ res_target, const unsigned char* __restrict__ active,
                                              const unsigned char* __restrict__ newState) {
  return r < R && res_target[r] == newest && active[r] != 0 && newState[r] == 0;
}
__device__ __forceinline__ void refBaCountBody(const int R, const int newest, const int* __restrict__ res_target, const unsigned char* __restrict__ active,
                                               const unsigned char* __restrict__ newState, const float* __restrict__ center, const int w0, const int h0,
                                               int* __restrict__ cnt, int* __restrict__ n_selected) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool sel = refBaSelected(r, R, newest, res_target, active, newState);
  if (sel) {
    const int pix = refPointPixel(center[3 * (size_t)r], center[3 * (size_t)r + 1], w0, h0);
    if (pix >= 0) atomicAdd(&cnt[pix], 1);
  }
  const unsigned long long m = __ballot(sel);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_selected, __popcll(m));
}
__device__ __forceinline__ void refBaScatterBody(const int R, const int newest, const int* __restrict__ res_point, const int* __restrict__ res_target,
                                                 const unsigned char* __restrict__ active, const unsigned char* __restrict__ newState,
                                                 const float* __restrict__ center, const float* __restrict__ HdiF, float* __restrict__ id0, float* __restrict__ ws0,
                                                 const int w0, const int h0, const int* __restrict__ cnt, int* __restrict__ n_crowded, int2* __restrict__ crowded,
                                                 const int cap) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (!refBaSelected(r, R, newest, res_target, active, newState)) return;
  const float* c3 = center + 3 * (size_t)r;
  const int pix = refPointPixel(c3[0], c3[1], w0, h0);
  if (pix < 0) return;
  if (cnt[pix] <= 2) {
    const float weight = refPointWeight(HdiF[res_point[r]]);
    atomicAdd(&id0[pix], c3[2] * weight);
    atomicAdd(&ws0[pix], weight);
  } else {
    const int k = atomicAdd(n_crowded, 1);
    if (k < cap) crowded[k] = make_int2(pix, r);
  }
}
__device__ __forceinline__ void refBaCrowdedBody(const int* __restrict__ res_point, const float* __restrict__ center, const float* __restrict__ HdiF,
                                                 float* __restrict__ id0, float* __restrict__ ws0, const int* __restrict__ n_crowded,
                                                 const int2* __restrict__ crowded, const int cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int L = min(*n_crowded, cap);
  if (i >= L) return;
  const int2 e = crowded[i];
  for (int j = 0; j < L; j++) { const int2 o = crowded[j]; if (o.x == e.x && o.y < e.y) return; }   // a lower index of this pixel owns it
  float a = id0[e.x], b = ws0[e.x];   // zero: (b) left a crowded pixel alone
  int last = -1;
  for (;;) {
    int r = 0x7fffffff;
    for (int j = 0; j < L; j++) { const int2 o = crowded[j]; if (o.x == e.x && o.y > last && o.y < r) r = o.y; }
    if (r == 0x7fffffff) break;
    const float weight = refPointWeight(HdiF[res_point[r]]);
    a += center[3 * (size_t)r + 2] * weight;
    b += weight;
    last = r;
  }
  id0[e.x] = a;
  ws0[e.x] = b;
}
__global__ void __launch_bounds__(256) k_ref_ba_count(const RefBaSrc S, const int w0, const int h0, int* __restrict__ cnt, int* __restrict__ n_selected) {
  refBaCountBody(S.R, S.newest, S.res_target, S.active, S.newState, S.center, w0, h0, cnt, n_selected);
}
__global__ void __launch_bounds__(256) k_ref_ba_scatter(const RefBaSrc S, float* __restrict__ id0, float* __restrict__ ws0, const int w0, const int h0,
                                                         const int* __restrict__ cnt, int* __restrict__ n_crowded, int2* __restrict__ crowded, const int cap) {
  refBaScatterBody(S.R, S.newest, S.res_point, S.res_target, S.active, S.newState, S.center, S.HdiF, id0, ws0, w0, h0, cnt, n_crowded, crowded, cap);
}
__global__ void __launch_bounds__(256) k_ref_ba_crowded(const RefBaSrc S, float* __restrict__ id0, float* __restrict__ ws0, const int* __restrict__ n_crowded,
                                                         const int2* __restrict__ crowded, const int cap) {
  refBaCrowdedBody(S.res_point, S.center, S.HdiF, id0, ws0, n_crowded, crowded, cap);
}

// nested 2x2 sums in the reference's operand order: ((a + b) + c) + d, level by level
template <int L>
__device__ __forceinline__ float pooledSum(const float* __restrict__ p0, const int w0, const int x, const int y) {
  if constexpr (L == 0) {
    return p0[x + y * w0];
  } else if constexpr (L <= 2) {
    return pooledSum<L - 1>(p0, w0, 2 * x, 2 * y) + pooledSum<L - 1>(p0, w0, 2 * x + 1, 2 * y) +
           pooledSum<L - 1>(p0, w0, 2 * x, 2 * y + 1) + pooledSum<L - 1>(p0, w0, 2 * x + 1, 2 * y + 1);
  } else {
    // from level 3 on the four children are visited by a ROLLED loop (same operand order): fully unrolled, level 5 issued its 1024 loads at once and took 256 VGPRs +
    // 62 AGPRs for a kernel that runs once per keyframe
    float t = 0.f;
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
      const float v = pooledSum<L - 1>(p0, w0, 2 * x + (q & 1), 2 * y + (q >> 1));
      t = q == 0 ? v : t + v;
    }
    return t;
  }
}

// all levels >= 1 in one launch; idx runs over the concatenated pixels of levels 1..L-1
__device__ __forceinline__ void refPoolBody(const RefLevels& R, float* __restrict__ idp, float* __restrict__ wsp) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x + R.off[1];
  if (idx >= R.total) return;
  int lvl = 1;
  while (lvl + 1 < R.levels && idx >= R.off[lvl + 1]) lvl++;
  const int li = (int)(idx - R.off[lvl]);
  const int x = li % R.w[lvl], y = li / R.w[lvl];
  float a, b;
  switch (lvl) {
    case 1: a = pooledSum<1>(idp, R.w[0], x, y); b = pooledSum<1>(wsp, R.w[0], x, y); break;
    case 2: a = pooledSum<2>(idp, R.w[0], x, y); b = pooledSum<2>(wsp, R.w[0], x, y); break;
    case 3: a = pooledSum<3>(idp, R.w[0], x, y); b = pooledSum<3>(wsp, R.w[0], x, y); break;
    case 4: a = pooledSum<4>(idp, R.w[0], x, y); b = pooledSum<4>(wsp, R.w[0], x, y); break;
    default: a = pooledSum<5>(idp, R.w[0], x, y); b = pooledSum<5>(wsp, R.w[0], x, y); break;
  }
  idp[idx] = a;
  wsp[idx] = b;
}
__global__ void __launch_bounds__(256) k_ref_pool(const RefLevels R, float* __restrict__ idp, float* __restrict__ wsp) { refPoolBody(R, idp, wsp); }

// dilation: reads the un-dilated planes (the reference's weightSums_bak + never-overwritten idepth
// entries), writes new planes — race free by construction.
__device__ __forceinline__ void refDilateBody(const RefLevels& R, const float* __restrict__ idp, const float* __restrict__ wsp,
                                              float* __restrict__ idp2, float* __restrict__ wsp2) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= R.total) return;
  int lvl = 0;
  while (lvl + 1 < R.levels && idx >= R.off[lvl + 1]) lvl++;
  const int wl = R.w[lvl], hl = R.h[lvl];
  const int i = (int)(idx - R.off[lvl]);
  const float* id = idp + R.off[lvl];
  const float* ws = wsp + R.off[lvl];
  float oid = id[i], ows = ws[i];
  const int wh = wl * hl - wl;
  if (i >= wl + 1 && i < wh - 1 && ows <= 0) {
    float sum = 0, num = 0, numn = 0;
    int n0, n1, n2, n3;
    if (lvl < 2) { n0 = i + 1 + wl; n1 = i - 1 - wl; n2 = i + wl - 1; n3 = i - wl + 1; }
    else         { n0 = i + 1;      n1 = i - 1;      n2 = i + wl;     n3 = i - wl; }
    if (ws[n0] > 0) { sum += id[n0]; num += ws[n0]; numn++; }
    if (ws[n1] > 0) { sum += id[n1]; num += ws[n1]; numn++; }
    if (ws[n2] > 0) { sum += id[n2]; num += ws[n2]; numn++; }
    if (ws[n3] > 0) { sum += id[n3]; num += ws[n3]; numn++; }
    if (numn > 0) { oid = sum / numn; ows = num / numn; }
  }
  idp2[idx] = oid;
  wsp2[idx] = ows;
}
__global__ void __launch_bounds__(256) k_ref_dilate(const RefLevels R, const float* __restrict__ idp, const float* __restrict__ wsp,
                                                     float* __restrict__ idp2, float* __restrict__ wsp2) {
  refDilateBody(R, idp, wsp, idp2, wsp2);
}

// normalise; returns whether pixel (x,y) of level lvl becomes a template point, and its record
__device__ __forceinline__ bool refPixel(const RefLevels& R, const int lvl, const int x, const int y, const float* __restrict__ idp2,
                                         const float* __restrict__ wsp2, const float* __restrict__ refI, float4& rec, float& idOut) {
  const int wl = R.w[lvl], hl = R.h[lvl];
  const int li = x + y * wl;
  const float idv = idp2[R.off[lvl] + li];
  idOut = idv;
  if (!(x >= 2 && x < wl - 2 && y >= 2 && y < hl - 2)) return false;
  const float wsv = wsp2[R.off[lvl] + li];
  if (wsv > 0) {
    const float idn = idv / wsv;
    const float color = refI[li];
    if (!isfinite(color) || !(idn > 0)) { idOut = -1; return false; }
    idOut = idn;
    rec = make_float4((float)x, (float)y, idn, color);
    return true;
  }
  idOut = -1;
  return false;
}

// workgroup = one 16x16 pixel block; wave k = 8x8 tile (k&1, k>>1) of the block; lane = (lx = l&7, ly = l>>3)
__device__ __forceinline__ void blockToPixel(const RefLevels& R, const int blk, int& lvl, int& x, int& y) {
  lvl = 0;
  while (lvl + 1 < R.levels && blk >= R.tile_off[lvl + 1]) lvl++;
  const int b = blk - R.tile_off[lvl];
  const int bx = b % R.blocks_x[lvl], by = b / R.blocks_x[lvl];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  x = bx * 16 + (wave & 1) * 8 + (lane & 7);
  y = by * 16 + (wave >> 1) * 8 + (lane >> 3);
}

// pass 1: per-block counts (+ per (row, 8-px segment) counts on level 0)
__device__ __forceinline__ void refCountBody(const RefLevels& R, const float* __restrict__ idp2, const float* __restrict__ wsp2,
                                             const FrameStore& fs, const int ref_slot, int* __restrict__ blk_count, int* __restrict__ seg_count) {
  int lvl, x, y;
  blockToPixel(R, blockIdx.x, lvl, x, y);
  bool flag = false;
  const bool inside = x < R.w[lvl] && y < R.h[lvl];
  if (inside) {
    float4 rec; float idn;
    flag = refPixel(R, lvl, x, y, idp2, wsp2, fs.level(ref_slot, lvl), rec, idn);
  }
  __shared__ int s_cnt[4];
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63;
  if (lane == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
  if (inside && (lane & 7) == 0) seg_count[R.seg_off[lvl] + y * R.seg_x[lvl] + (x >> 3)] = __popcll((m >> (lane & 56)) & 0xffull);
  __syncthreads();
  if (threadIdx.x == 0) blk_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}
__global__ void __launch_bounds__(256) k_ref_count(const RefLevels R, const float* __restrict__ idp2, const float* __restrict__ wsp2,
                                                    const FrameStore fs, const int ref_slot, int* __restrict__ blk_count, int* __restrict__ seg_count) {
  refCountBody(R, idp2, wsp2, fs, ref_slot, blk_count, seg_count);
}

// block-wide exclusive scan helper over 1024 threads (value per thread) ; returns exclusive prefix, total via s_total
__device__ __forceinline__ int scan1024(const int c, int* s_wave, int& total) {
  int v = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if ((int)(threadIdx.x & 63) >= d) v += o;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  int woff = 0, tot = 0;
  for (int k = 0; k < 16; k++) { const int sv = s_wave[k]; if (k < (int)(threadIdx.x >> 6)) woff += sv; tot += sv; }
  total = tot;
  return woff + v - c;
}

// pass 2: blockIdx.x < levels: exclusive scan of the block counts of that level -> blk_base, pc_n[lvl].
//         blockIdx.x >= levels: row-major rank tables of level blockIdx.x - levels: seg_count -> exclusive prefix in row-major order (in place).
// pc_n_row (may be NULL): a second place for pc_n[lvl], the window's row of a batch's [W][levels] table
__device__ __forceinline__ void refScanBody(const RefLevels& R, const int* __restrict__ blk_count, int* __restrict__ blk_base,
                                            int* __restrict__ pc_n, int* __restrict__ seg_count, int* __restrict__ pc_n_row) {
  __shared__ int s_wave[16];
  int carry = 0;
  if ((int)blockIdx.x < R.levels) {
    const int lvl = blockIdx.x;
    const int t0 = R.tile_off[lvl], t1 = R.tile_off[lvl + 1];
    for (int base = t0; base < t1; base += 1024) {
      const int t = base + threadIdx.x;
      const int c = (t < t1) ? blk_count[t] : 0;
      int total;
      const int ex = scan1024(c, s_wave, total);
      if (t < t1) blk_base[t] = carry + ex;
      carry += total;
    }
    if (threadIdx.x == 0) { pc_n[lvl] = carry; if (pc_n_row) pc_n_row[lvl] = carry; }
  } else {
    const int lvl = blockIdx.x - R.levels;
    const int n = R.h[lvl] * R.seg_x[lvl];  // row-major (y, segment) order == raster order of the segments
    int* sc = seg_count + R.seg_off[lvl];
    for (int base = 0; base < n; base += 1024) {
      const int t = base + threadIdx.x;
      const int c = (t < n) ? sc[t] : 0;
      int total;
      const int ex = scan1024(c, s_wave, total);
      if (t < n) sc[t] = carry + ex;
      carry += total;
    }
  }
}
__global__ void __launch_bounds__(1024) k_ref_scan(const RefLevels R, const int* __restrict__ blk_count, int* __restrict__ blk_base,
                                                    int* __restrict__ pc_n, int* __restrict__ seg_count) {
  refScanBody(R, blk_count, blk_base, pc_n, seg_count, nullptr);
}

// pass 3: ranked write of the template records in tile order, the dense normalised idepth map (debugPlotIDepthMap)
// and, on level 0, the flow-sample bit of every entry whose ROW-MAJOR rank is a multiple of 32.
// GL = false, the single-window kernel: the storage order is R.order and the entry pc[lvl] a generic pointer (its one flat store).  GL = true, the W-window kernel: the
// order is `win_order`, from the window's record (the geometry it is handed is the context's, the order the tracker's), and pc[lvl] is read as a global pointer
// (ba_batch_kernels.hpp: gl()).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wincompatible-pointer-types-discards-qualifiers"
template <bool GL>
__device__ __forceinline__ void refWriteBody(const RefLevels& R, const int win_order, const float* __restrict__ idp2, const float* __restrict__ wsp2,
                                             const FrameStore& fs, const int ref_slot, const int* __restrict__ blk_base,
                                             const int* __restrict__ seg_prefix, float4* const* __restrict__ pc,
                                             float* __restrict__ idepth_dense, unsigned long long* __restrict__ flow_mask) {
  int lvl, x, y;
  blockToPixel(R, blockIdx.x, lvl, x, y);
  bool flag = false;
  float4 rec = make_float4(0, 0, 0, 0);
  float idn = -1;
  const bool inside = x < R.w[lvl] && y < R.h[lvl];
  if (inside) flag = refPixel(R, lvl, x, y, idp2, wsp2, fs.level(ref_slot, lvl), rec, idn);
  __shared__ int s_cnt[4];
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_cnt[wave] = __popcll(m);
  __syncthreads();
  int woff = 0;
  for (int k = 0; k < wave; k++) woff += s_cnt[k];
  if (flag) {
    const unsigned long long rowbits = (m >> (lane & 56)) & 0xffull;
    const int raster = seg_prefix[R.seg_off[lvl] + y * R.seg_x[lvl] + (x >> 3)] + __popcll(rowbits & ((1ull << (lane & 7)) - 1ull));   // rank in the reference's row-major list
    const int pos = (GL ? win_order : R.order) ? raster : blk_base[blockIdx.x] + woff + __popcll(m & ((1ull << lane) - 1ull));
    if constexpr (GL) ((float4*)(*reinterpret_cast<__attribute__((address_space(1))) float4* const*>(&pc[lvl])))[pos] = rec;
    else pc[lvl][pos] = rec;
    if (lvl == 0 && (raster & 31) == 0) atomicOr(&flow_mask[pos >> 6], 1ull << (pos & 63));
  }
  if (inside) idepth_dense[R.off[lvl] + x + y * R.w[lvl]] = idn;
}
#pragma clang diagnostic pop
__global__ void __launch_bounds__(256) k_ref_write(const RefLevels R, const float* __restrict__ idp2, const float* __restrict__ wsp2,
                                                    const FrameStore fs, const int ref_slot, const int* __restrict__ blk_base,
                                                    const int* __restrict__ seg_prefix, float4* const* __restrict__ pc,
                                                    float* __restrict__ idepth_dense, unsigned long long* __restrict__ flow_mask) {
  refWriteBody<false>(R, 0, idp2, wsp2, fs, ref_slot, blk_base, seg_prefix, pc, idepth_dense, flow_mask);
}

}  // namespace dmv
