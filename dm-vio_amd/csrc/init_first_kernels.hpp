// CoarseInitializer::setFirst on the device (include/dmvio_hip_init_first.h): the coarse selector of the levels >= 1 (makePixelStatus / gridMaxSelection,
// src/dso/FullSystem/PixelSelector.h:40-253), the raster-ordered point lists (CoarseInitializer.cpp:834-872) and makeNN's two searches (:1001-1078).
//   k_first_grid_select   thread per pot x pot cell: the four directional maxima of the cell, flagged in the byte map; the count of distinct flagged pixels
//   k_first_scanA/B/C     raster-order compaction of the flagged pixels of setFirst's window into (u, v, my_type): tile sums, one workgroup over the sums, tiles
//   k_first_knn<K, HALF>  K nearest candidates of every query under (float distance, index), nearest first; K = 10 on the level itself, K = 1 with the halved query
//                         against the level above (the parent)
// No kernel waits on another workgroup; the only atomics are integer adds.
#pragma once
#include "common.h"
#include "interp.hpp"

namespace dmv {

enum { FIRST_TILE = 1024 };   // pixels per scan tile (256 threads x 4)
enum { FIRST_KNN_WG = 256 };  // queries of a workgroup = candidates of a tile

// gridMaxSelection (PixelSelector.h:40-196): `pot` at run time covers the templated forms and the generic one, which differ in nothing else.  Cells start at x, y = 1 and
// step by pot while < w - pot / < h - pot (no partial cells); inside a cell dx is the outer loop and dy the inner one, every comparison strict, so among equal values the
// first in that order wins.  A cell's four winners may coincide: a cell adds the number of DISTINCT winners, and cells do not overlap, so the sum is the reference's numGood.
__global__ void __launch_bounds__(256) k_first_grid_select(const float* __restrict__ I, const int w, const int h, const int pot, const float THFac, const int ncx, const int ncy,
                                                           unsigned char* __restrict__ map, int* __restrict__ count) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  int good = 0;
  if (c < ncx * ncy) {
    const int x0 = 1 + (c % ncx) * pot, y0 = 1 + (c / ncx) * pot;
    const float TH = THFac * 10.0f * 0.75f;   // THFac * minUseGrad_pixsel * (0.75f), :65
    const float TH2 = TH * TH;
    float bestXX = 0.f, bestYY = 0.f, bestXY = 0.f, bestYX = 0.f;
    int idXX = -1, idYY = -1, idXY = -1, idYX = -1;
    for (int dx = 0; dx < pot; dx++)
      for (int dy = 0; dy < pot; dy++) {
        const float2 g = gradAt(I, w, h, x0 + dx, y0 + dy);   // 1 <= x <= w - 2, 1 <= y <= h - 2
        const float sqgd = g.x * g.x + g.y * g.y;
        if (sqgd > TH2) {
          const int idx = dx + dy * w;
          const float agx = fabsf(g.x), agy = fabsf(g.y), gxpy = fabsf(g.x - g.y), gxmy = fabsf(g.x + g.y);
          if (agx > bestXX) { bestXX = agx; idXX = idx; }
          if (agy > bestYY) { bestYY = agy; idYY = idx; }
          if (gxpy > bestXY) { bestXY = gxpy; idXY = idx; }
          if (gxmy > bestYX) { bestYX = gxmy; idYX = idx; }
        }
      }
    unsigned char* map0 = map + x0 + y0 * w;
    if (idXX >= 0) { map0[idXX] = 1; good++; }
    if (idYY >= 0) { map0[idYY] = 1; good += idYY != idXX; }
    if (idXY >= 0) { map0[idXY] = 1; good += idXY != idXX && idXY != idYY; }
    if (idYX >= 0) { map0[idYX] = 1; good += idYX != idXX && idYX != idYY && idYX != idXY; }
  }
  // integer sum: wave, workgroup through LDS, one atomic per workgroup
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) good += __shfl_xor(good, off, 64);
  if ((threadIdx.x & 63) == 0 && good) atomicAdd(&s_n, good);
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(count, s_n);
}

// ---- the raster-ordered point list of a level (:834-872): the flagged pixels with 3 <= x < w - 4, 3 <= y < h - 4
__device__ __forceinline__ int firstFlag(const unsigned char* __restrict__ map, const int w, const int h, const int i) {
  if (i >= w * h || map[i] == 0) return 0;
  const int x = i % w, y = i / w;
  return x >= 3 && x < w - 4 && y >= 3 && y < h - 4;
}
// inclusive scan over the workgroup's 256 threads; *total = the workgroup's sum
__device__ __forceinline__ int firstBlockScan(int v, int* total) {
  __shared__ int s_w[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  __syncthreads();   // s_w of a previous call has been read
  if (lane == 63) s_w[wv] = v;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int s = s_w[k];
    if (k < wv) before += s;
    all += s;
  }
  *total = all;
  return v + before;
}
__global__ void __launch_bounds__(256) k_first_scanA(const unsigned char* __restrict__ map, const int w, const int h, int* __restrict__ tiles) {
  const int base = blockIdx.x * FIRST_TILE + threadIdx.x * 4;
  int s = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) s += firstFlag(map, w, h, base + k);
  int total;
  firstBlockScan(s, &total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}
// one workgroup: tile sums -> exclusive, in place; the total into *n_out
__global__ void __launch_bounds__(256) k_first_scanB(int* __restrict__ tiles, const int ntiles, int* __restrict__ n_out) {
  int carry = 0;
  for (int base = 0; base < ntiles; base += 256) {
    const int i = base + threadIdx.x;
    const int v = i < ntiles ? tiles[i] : 0;
    int total;
    const int inc = firstBlockScan(v, &total);
    if (i < ntiles) tiles[i] = carry + inc - v;
    carry += total;
  }
  if (threadIdx.x == 0) *n_out = carry;
}
// u = (float)(x + 0.1): the addition in double, as :841-842.  my_type: the map's value where `typed` (level 0), else 1.  Writes at most `cap` points.
__global__ void __launch_bounds__(256) k_first_scanC(const unsigned char* __restrict__ map, const int w, const int h, const int* __restrict__ tiles, const int typed,
                                                     const int cap, float* __restrict__ u, float* __restrict__ v, float* __restrict__ my_type) {
  const int base = blockIdx.x * FIRST_TILE + threadIdx.x * 4;
  int f[4], s = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) { f[k] = firstFlag(map, w, h, base + k); s += f[k]; }
  int total;
  const int inc = firstBlockScan(s, &total);
  int at = tiles[blockIdx.x] + inc - s;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (f[k] && at < cap) {
      const int i = base + k;
      u[at] = (float)((double)(i % w) + 0.1);
      v[at] = (float)((double)(i / w) + 0.1);
      my_type[at] = typed ? (float)map[i] : 1.0f;
    }
    at += f[k];
  }
}

// ---- makeNN's searches (:1032-1068), by a rule of the library's own (the header says why): the K smallest candidates under (distance, index), nearest first, with
// FLANNPointcloud's distance (CoarseInitializer.h:177-182) in float: d0 = q0 - u, d1 = q1 - v, d0 * d0 + d1 * d1, no contraction.
//
// A workgroup serves 256 consecutive queries and walks the candidates in tiles of 256 consecutive indices, staged through LDS, outward in both directions from the tile
// that holds the first candidate whose v is not below the v of the workgroup's first query.  Every thread keeps its K pairs sorted in registers (static indices only).
//
// Termination.  The caller guarantees cv non-decreasing in the index (raster order).  Let vmax / vmin bound the query v of the workgroup's live threads and D the largest
// current K-th distance among them (+inf while any list is not full).  Upward, tile t starts at candidate f with cv[f] >= vmax when g = fl(cv[f] - vmax) >= 0.  For any
// live query q and any candidate c with index >= f: cv[c] >= cv[f] and qv <= vmax, so cv[c] - qv >= cv[f] - vmax >= 0 in exact arithmetic; rounding to nearest is monotone
// and symmetric, so |d1| = |fl(qv - cv[c])| >= g.  Products and sums of non-negative floats are monotone under rounding too: fl(d1 * d1) >= fl(g * g), and
// fl(fl(d0 * d0) + fl(d1 * d1)) >= fl(0 + fl(d1 * d1)) = fl(d1 * d1).  Hence the FLOAT distance of every such pair is >= B = fl(g * g).  A candidate enters a list only if
// (d, index) < (K-th distance, its index); with B > D (strict) it has d >= B > D >= the list's K-th distance and cannot, whatever its index.  So the direction ends for
// the whole workgroup, for this tile and all beyond it.  Downward the same with the tile's LAST candidate l, g = fl(vmin - cv[l]) and candidates of index <= l.
// Neither D grows nor the gap shrinks as the walk goes on, so an ended direction stays ended.  A direction also ends where the tiles run out.
template <int K>
__device__ __forceinline__ void firstInsert(float (&dist)[K], int (&idx)[K], const float d, const int j) {
  if (d < dist[K - 1] || (d == dist[K - 1] && j < idx[K - 1])) {
    dist[K - 1] = d; idx[K - 1] = j;
#pragma unroll
    for (int k = K - 1; k > 0; k--) {
      const bool lt = dist[k] < dist[k - 1] || (dist[k] == dist[k - 1] && idx[k] < idx[k - 1]);
      const float td = dist[k]; const int ti = idx[k];
      dist[k] = lt ? dist[k - 1] : td; idx[k] = lt ? idx[k - 1] : ti;
      dist[k - 1] = lt ? td : dist[k - 1]; idx[k - 1] = lt ? ti : idx[k - 1];
    }
  }
}
// max (WANT_MAX) or min over the workgroup's 256 threads, through s_r[4]
template <bool WANT_MAX>
__device__ __forceinline__ float firstBlockReduce(float v, float* s_r) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float o = __shfl_xor(v, off, 64);
    v = WANT_MAX ? fmaxf(v, o) : fminf(v, o);
  }
  __syncthreads();   // s_r of a previous call has been read
  if ((threadIdx.x & 63) == 0) s_r[threadIdx.x >> 6] = v;
  __syncthreads();
  const float a = s_r[0], b = s_r[1], c = s_r[2], d = s_r[3];
  return WANT_MAX ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : fminf(fminf(a, b), fminf(c, d));
}
// HALF: the query is (u * 0.5f - 0.25f, v * 0.5f - 0.25f) of the lower level's point (:1056: a float multiply, then a float subtract).  out: K ints per query.
template <int K, bool HALF>
__global__ void __launch_bounds__(FIRST_KNN_WG) k_first_knn(const int nq, const float* __restrict__ qu_, const float* __restrict__ qv_, const int nc,
                                                            const float* __restrict__ cu, const float* __restrict__ cv, int* __restrict__ out) {
  __shared__ float s_u[FIRST_KNN_WG], s_v[FIRST_KNN_WG], s_r[4];
  __shared__ int s_start;
  const int q = blockIdx.x * FIRST_KNN_WG + threadIdx.x;
  const bool live = q < nq;
  float qu = 0.f, qv = 0.f;
  if (live) {
    qu = qu_[q]; qv = qv_[q];
    if (HALF) { qu = qu * 0.5f - 0.25f; qv = qv * 0.5f - 0.25f; }
  }
  const float INF = __builtin_inff();
  const float vmax = firstBlockReduce<true>(live ? qv : -INF, s_r);
  const float vmin = firstBlockReduce<false>(live ? qv : INF, s_r);
  if (threadIdx.x == 0) {   // thread 0 is live (the grid has no empty workgroup): the first candidate with cv >= its qv
    int lo = 0, hi = nc;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cv[mid] < qv) lo = mid + 1; else hi = mid; }
    s_start = lo;
  }
  __syncthreads();
  const int ntiles = (nc + FIRST_KNN_WG - 1) / FIRST_KNN_WG;
  const int t0 = min(s_start / FIRST_KNN_WG, ntiles - 1);
  float dist[K]; int idx[K];
#pragma unroll
  for (int k = 0; k < K; k++) { dist[k] = INF; idx[k] = 0x7fffffff; }
  int up = t0, down = t0 - 1;   // the next tile of either direction; up >= ntiles / down < 0: ended
  while (up < ntiles || down >= 0) {
    // the workgroup's largest K-th distance (a dead thread asks for nothing)
    const float D = firstBlockReduce<true>(live ? dist[K - 1] : -INF, s_r);
    if (up < ntiles) {
      const float g = cv[up * FIRST_KNN_WG] - vmax;
      if (g >= 0.f && g * g > D) up = ntiles;
    }
    if (down >= 0) {
      const float g = vmin - cv[min(nc, (down + 1) * FIRST_KNN_WG) - 1];
      if (g >= 0.f && g * g > D) down = -1;
    }
#pragma unroll 1
    for (int dir = 0; dir < 2; dir++) {
      const int t = dir == 0 ? up : down;
      if (t < 0 || t >= ntiles) continue;   // uniform over the workgroup
      const int base = t * FIRST_KNN_WG, m = min(FIRST_KNN_WG, nc - base);
      __syncthreads();   // the tile before has been read
      if ((int)threadIdx.x < m) { s_u[threadIdx.x] = cu[base + threadIdx.x]; s_v[threadIdx.x] = cv[base + threadIdx.x]; }
      __syncthreads();
      if (live)
        for (int j = 0; j < m; j++) {
          const float d0 = qu - s_u[j], d1 = qv - s_v[j];
          firstInsert<K>(dist, idx, d0 * d0 + d1 * d1, base + j);
        }
      if (dir == 0) up++; else down--;
    }
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < K; k++) out[(size_t)q * K + k] = idx[k];
  }
}

}  // namespace dmv
