// Pixel selection on the device: PixelSelector::makeMaps (src/dso/FullSystem/PixelSelector2.cpp:158-307) with makeHists (:94-157) and select (:311-454).
//
// select() is one sequential walk (4pot blocks in raster order, inside them 2pot blocks, inside them pot cells, inside them pixels).  What it computes, derived from the
// code (line numbers of PixelSelector2.cpp):
//   * a pot cell selects at level 0 iff one of its pixels has ag0 > pixelTH0*thFactor AND |grad . dir2| > 0 (:394-401; bestVal2 starts at 0, the test is strict), where
//     dir2 = directions[randomPattern[n2] & 15] and n2 = the number of level-0 selections made before the cell starts (:376).  The selected pixel is the arg-max of
//     |grad . dir2| over the passing pixels, the FIRST one in walk order among equals (strict '>').
//   * the first level-0 best of a 2pot block sets bestIdx3 = -2, and :403 skips the level-1 test for every later pixel of the block; bestIdx3 is never written again,
//     so :437 finds no level-1 point.  Pixels before it did compete, but their candidate is the one overwritten.  Hence: a 2pot block yields a level-1 point iff NONE
//     of its cells selects at level 0, and then every pixel of the block competes (ag1 > pixelTH1*thFactor, arg-max of |grad . dir3| > 0, first in walk order).  In
//     such a block n2 does not move, so dir3 (:368, n2 at the block's start) is the direction of n2 at any of its cells.
//   * likewise bestIdx4 = -2 is set by the first level-0 best (:401) or level-1 best (:413) of a 4pot block: it yields a level-2 point iff it has no level-0 and no
//     level-1 point, all its pixels compete, dir4 from n2 at its start (:360).
//   * only level 0 feeds n2: n2 at a cell is an exclusive prefix count, over the walk order, of "the cell selects under the direction its own n2 draws" — a recurrence.
//
// Decomposition (every phase is its own launch; nothing waits inside a launch; order comes from scans, the atomics used are OR / MAX / integer ADD, whose result does
// not depend on arrival order):
//   k_sel_absgrad        absSquaredGrad of levels 0..2 (as k_abs_squared_grad, image_kernels.hpp) into the handle's scratch
//   k_sel_hist, _smooth  makeHists: one workgroup per 16x16 block (50-bin histogram in LDS, quantile), 3x3 mean squared
//   k_sel_cellmask       thread per pixel: the 16-bit mask "this pixel makes its cell select under direction d", OR-ed into the cell's word
//   k_sel_scanA/B/C      n2 at every cell: exclusive scan of (mask != 0) over the cells stored in walk order (two-level: tile sums, one workgroup over the sums, tiles)
//   k_sel_scan_exact     only when a mask is neither 0 nor 0xFFFF ("mixed": the cell's selection depends on the direction): the recurrence
//                        n2 += (mask[cell] >> (randomPattern[n2] & 15)) & 1 on one wave, 64 cells per step, direction-free groups added by their popcount
//   k_sel_pick           thread per pixel: 64-bit (value, ~walk rank) keys MAX-ed into its cell (level 0), 2pot block (level 1) and 4pot block (level 2)
//   k_sel_write          thread per cell: decodes the keys into the status map, counts n3 / n4
//   k_sel_scanA/B/C      raster-order scans of the map: the random sub-selection's running count (:250-264), then the compacted (u, v, type) list and the list
//                        restricted to the window FullSystem::makeNewTraces walks (FullSystem.cpp:1653-1654)
// Every kernel's body is a __device__ function (selAbsgradBody ... selWriteBody) that the batched forms of select_batch_kernels.hpp call as well.
// Cells are stored in a PADDED walk order: cell (cx, cy) of the pot grid lives at ((by4*nb4x + bx4)*4 + sub3)*4 + sub2, cells the image clips away keep mask 0.
#pragma once
#include "common.h"
#include "interp.hpp"

namespace dmv {

// PixelSelector2.cpp:328-344
static __constant__ float c_selDirs[16][2] = {{0.f, 1.0000f},      {0.3827f, 0.9239f},  {0.1951f, 0.9808f},  {0.9239f, 0.3827f},  {0.7071f, 0.7071f}, {0.3827f, -0.9239f},
                                              {0.8315f, 0.5556f},  {0.8315f, -0.5556f}, {0.5556f, -0.8315f}, {0.9808f, 0.1951f},  {0.9239f, -0.3827f}, {0.7071f, -0.7071f},
                                              {0.5556f, 0.8315f},  {0.9808f, -0.1951f}, {1.0000f, 0.0000f},  {0.1951f, -0.9808f}};

struct SelGeom {
  int w, h, w1, w2;
  int pot;           // geometry potential: min(currentPotential, max(w, h)) — one cell covers the image beyond that
  int nb4x, ncell;   // 4pot blocks per row; padded cell count = 16 * nb4x * nb4y
  int nbW;           // thsStep
  float thFactor, dw1, dw2;
  int useDir;        // setting_selectDirectionDistribution
};

enum { SEL_TILE = 1024 };   // elements per scan tile (256 threads x 4)
enum { SEL_EXACT_AHEAD = 8 };   // k_sel_scan_exact: groups of 64 cells whose masks are in flight together
// slots of the handle's small counter block
enum { SELC_N2 = 0, SELC_N3, SELC_N4, SELC_EXACT, SELC_NSEL, SELC_NWIN, SELC_MIXED, SELC_NZ, SELC_COUNT = 16 };

__device__ __forceinline__ float selDirNorm(const float2 g, const int d) { return fabsf(g.x * c_selDirs[d][0] + g.y * c_selDirs[d][1]); }
// :385
__device__ __forceinline__ bool selInside(const SelGeom& G, const int x, const int y) { return !(x < 4 || x >= G.w - 5 || y < 4 || y > G.h - 4); }
__device__ __forceinline__ int selCellOf(const SelGeom& G, const int x, const int y, unsigned int* rank) {
  const int cx = x / G.pot, cy = y / G.pot;
  *rank = (unsigned int)(y - cy * G.pot) * (unsigned int)G.pot + (unsigned int)(x - cx * G.pot);
  return (((cy >> 2) * G.nb4x + (cx >> 2)) * 4 + (((cy >> 1) & 1) * 2 + ((cx >> 1) & 1))) * 4 + ((cy & 1) * 2 + (cx & 1));
}
__device__ __forceinline__ void selCellOrigin(const SelGeom& G, const int c, int* x0, int* y0) {
  const int b4 = c >> 4, s3 = (c >> 2) & 3, s2 = c & 3;
  *x0 = ((b4 % G.nb4x) * 4 + (s3 & 1) * 2 + (s2 & 1)) * G.pot;
  *y0 = ((b4 / G.nb4x) * 4 + (s3 >> 1) * 2 + (s2 >> 1)) * G.pot;
}
__device__ __forceinline__ unsigned long long selKey(const float v, const unsigned int rank) {
  return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - rank);
}
__device__ __forceinline__ void selKeyMax(unsigned long long* p, const unsigned long long k) {
  // MAX is monotone: a stale read only costs an atomic that changes nothing
  if (__atomic_load_n(p, __ATOMIC_RELAXED) < k) atomicMax(p, k);
}

// absSquaredGrad[0..2] of FrameHessian::makeImages (HessianBlocks.cpp:169-189), the arithmetic of k_abs_squared_grad; out = [level 0 | level 1 | level 2]
__device__ __forceinline__ void selAbsgradBody(const float* __restrict__ I0, const float* __restrict__ I1, const float* __restrict__ I2, const int w0, const int h0,
                                               const int w1, const int h1, const int w2, const int h2, const float* __restrict__ B, float* __restrict__ out) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int n0 = w0 * h0, n1 = w1 * h1, n2 = w2 * h2;
  if (gid >= n0 + n1 + n2) return;
  const float* I = I0; int w = w0, h = h0, idx = gid;
  if (gid >= n0 + n1) { I = I2; w = w2; h = h2; idx = gid - n0 - n1; }
  else if (gid >= n0) { I = I1; w = w1; h = h1; idx = gid - n0; }
  float v = 0.f;
  if (idx >= w && idx < w * (h - 1)) {
    const float2 g = gradAt(I, w, h, idx % w, idx / w);
    v = g.x * g.x + g.y * g.y;
    if (B) {
      int c = (int)(I[idx] + 0.5f);
      if (c < 5) c = 5;
      if (c > 250) c = 250;
      const float gw = B[c + 1] - B[c];
      v *= gw * gw;
    }
  }
  out[gid] = v;
}
__global__ void __launch_bounds__(256) k_sel_absgrad(const float* __restrict__ I0, const float* __restrict__ I1, const float* __restrict__ I2, const int w0, const int h0,
                                                     const int w1, const int h1, const int w2, const int h2, const float* __restrict__ B, float* __restrict__ out) {
  selAbsgradBody(I0, I1, I2, w0, h0, w1, h1, w2, h2, B, out);
}

// makeHists, first loop (:106-125) + computeHistQuantil (:82-91): one workgroup per 16x16 block
__device__ __forceinline__ void selHistBody(const float* __restrict__ ag0, const int w, const int h, const int nbW, const float histCut, const float histAdd,
                                            float* __restrict__ ths) {
  __shared__ int s_hist[50];
  const int bx = blockIdx.x % nbW, by = blockIdx.x / nbW;
  if (threadIdx.x < 50) s_hist[threadIdx.x] = 0;
  __syncthreads();
  const int it = bx * 16 + (threadIdx.x & 15), jt = by * 16 + (threadIdx.x >> 4);
  if (!(it > w - 2 || jt > h - 2 || it < 1 || jt < 1)) {
    int g = (int)sqrtf(ag0[it + jt * w]);
    if (g > 48) g = 48;
    atomicAdd(&s_hist[g + 1], 1);
    atomicAdd(&s_hist[0], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int th = (int)(s_hist[0] * histCut + 0.5f);
    int q = 90;
    for (int i = 0; i < 90; i++) {
      // the reference walks hist[1..90] of a block of which it cleared 50 ints; with minGradHistCut < 1 and more than one pixel counted the walk ends inside them
      th -= (i + 1 < 50) ? s_hist[i + 1] : 0;
      if (th < 0) { q = i; break; }
    }
    ths[blockIdx.x] = q + histAdd;
  }
}
__global__ void __launch_bounds__(256) k_sel_hist(const float* __restrict__ ag0, const int w, const int h, const int nbW, const float histCut, const float histAdd,
                                                  float* __restrict__ ths) {
  selHistBody(ag0, w, h, nbW, histCut, histAdd, ths);
}

// makeHists, second loop (:127-151): the sum order of the reference
__device__ __forceinline__ void selSmoothBody(const float* __restrict__ ths, const int w32, const int h32, float* __restrict__ thsSmoothed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w32 * h32) return;
  const int x = i % w32, y = i / w32;
  float sum = 0, num = 0;
  if (x > 0) {
    if (y > 0) { num++; sum += ths[x - 1 + (y - 1) * w32]; }
    if (y < h32 - 1) { num++; sum += ths[x - 1 + (y + 1) * w32]; }
    num++; sum += ths[x - 1 + y * w32];
  }
  if (x < w32 - 1) {
    if (y > 0) { num++; sum += ths[x + 1 + (y - 1) * w32]; }
    if (y < h32 - 1) { num++; sum += ths[x + 1 + (y + 1) * w32]; }
    num++; sum += ths[x + 1 + y * w32];
  }
  if (y > 0) { num++; sum += ths[x + (y - 1) * w32]; }
  if (y < h32 - 1) { num++; sum += ths[x + (y + 1) * w32]; }
  num++; sum += ths[x + y * w32];
  thsSmoothed[i] = (sum / num) * (sum / num);
}
__global__ void __launch_bounds__(256) k_sel_smooth(const float* __restrict__ ths, const int w32, const int h32, float* __restrict__ thsSmoothed) {
  selSmoothBody(ths, w32, h32, thsSmoothed);
}

// bit d of a cell's mask: some pixel of the cell passes the level-0 threshold and scores > 0 against direction d
__device__ __forceinline__ void selCellmaskBody(const float* __restrict__ I, const float* __restrict__ ag0, const float* __restrict__ thsS, const SelGeom& G,
                                                unsigned int* __restrict__ mask) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned int m = 0;
  int c = -1;
  if (idx < G.w * G.h) {
    const int x = idx % G.w, y = idx / G.w;
    unsigned int rank;
    c = selCellOf(G, x, y, &rank);
    if (selInside(G, x, y)) {
      const float a = ag0[idx];
      if (a > thsS[(x >> 4) + (y >> 4) * G.nbW] * G.thFactor) {
        if (G.useDir) {
          const float2 g = gradAt(I, G.w, G.h, x, y);
#pragma unroll
          for (int d = 0; d < 16; d++) m |= (selDirNorm(g, d) > 0.f ? 1u : 0u) << d;
        } else {
          m = a > 0.f ? 0xFFFFu : 0u;
        }
      }
    }
  }
  // a wave that lies inside one cell (pot >= 64, or a short cell row) sends one OR
  const int c0 = __builtin_amdgcn_readfirstlane(c);
  if (__ballot(c != c0) == 0ull) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m |= (unsigned int)__shfl_xor((int)m, off, 64);
    if ((threadIdx.x & 63) == 0 && m && c0 >= 0) atomicOr(&mask[c0], m);
  } else if (m) {
    atomicOr(&mask[c], m);
  }
}
__global__ void __launch_bounds__(256) k_sel_cellmask(const float* __restrict__ I, const float* __restrict__ ag0, const float* __restrict__ thsS, const SelGeom G,
                                                      unsigned int* __restrict__ mask) {
  selCellmaskBody(I, ag0, thsS, G, mask);
}

// ---- two-level exclusive scans of two counters per element.  MODE_CELL: (cell selects, cell is mixed) over the padded walk order; MODE_NZ: (map != 0, -) in raster
// order; MODE_SURV: (survives the sub-selection, survives and lies in the makeNewTraces window) in raster order.
enum { SEL_MODE_CELL = 0, SEL_MODE_NZ = 1, SEL_MODE_SURV = 2 };
struct SelScanArgs {
  int n;              // elements
  int charTH, w, h;   // SURV (rn == NULL: no sub-selection)
};
template <int MODE> __device__ __forceinline__ int2 selScanVal(const SelScanArgs& A, const unsigned int* __restrict__ mask, const unsigned char* __restrict__ map,
                                                               const int* __restrict__ rn, const unsigned char* __restrict__ pattern, const int i) {
  if (i >= A.n) return make_int2(0, 0);
  if (MODE == SEL_MODE_CELL) {
    const unsigned int m = mask[i];
    return make_int2(m != 0u, m != 0u && m != 0xFFFFu);
  }
  if (MODE == SEL_MODE_NZ) return make_int2(map[i] != 0, 0);
  if (map[i] == 0) return make_int2(0, 0);
  if (rn && (int)pattern[rn[i]] > A.charTH) return make_int2(0, 0);   // :257
  const int x = i % A.w, y = i / A.w;
  return make_int2(1, x >= 3 && x < A.w - 4 && y >= 3 && y < A.h - 4);   // patternPadding+1 <= x < w-patternPadding-2 (FullSystem.cpp:1653-1654)
}
__device__ __forceinline__ int2 selAdd(const int2 a, const int2 b) { return make_int2(a.x + b.x, a.y + b.y); }
// inclusive scan over the workgroup's 256 threads; *total = the workgroup's sum
__device__ __forceinline__ int2 selBlockScan(int2 v, int2* total) {
  __shared__ int2 s_w[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int ox = __shfl_up(v.x, off, 64), oy = __shfl_up(v.y, off, 64);
    if (lane >= off) { v.x += ox; v.y += oy; }
  }
  __syncthreads();   // s_w of a previous call has been read
  if (lane == 63) s_w[wv] = v;
  __syncthreads();
  int2 before = make_int2(0, 0), all = make_int2(0, 0);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int2 s = s_w[k];
    if (k < wv) before = selAdd(before, s);
    all = selAdd(all, s);
  }
  *total = all;
  return selAdd(v, before);
}

template <int MODE> __device__ __forceinline__ void selScanABody(const SelScanArgs& A, const unsigned int* __restrict__ mask, const unsigned char* __restrict__ map,
                                                                 const int* __restrict__ rn, const unsigned char* __restrict__ pattern, int2* __restrict__ tiles) {
  const int base = blockIdx.x * SEL_TILE + threadIdx.x * 4;
  int2 s = make_int2(0, 0);
#pragma unroll
  for (int k = 0; k < 4; k++) s = selAdd(s, selScanVal<MODE>(A, mask, map, rn, pattern, base + k));
  int2 total;
  selBlockScan(s, &total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}
template <int MODE> __global__ void __launch_bounds__(256) k_sel_scanA(const SelScanArgs A, const unsigned int* __restrict__ mask, const unsigned char* __restrict__ map,
                                                                        const int* __restrict__ rn, const unsigned char* __restrict__ pattern, int2* __restrict__ tiles) {
  selScanABody<MODE>(A, mask, map, rn, pattern, tiles);
}
// one workgroup: tile sums -> exclusive, in place; the totals into counters[slot_x] / [slot_y] (slot < 0: not stored)
__device__ __forceinline__ void selScanBBody(int2* __restrict__ tiles, const int ntiles, int* __restrict__ counters, const int slot_x, const int slot_y) {
  int2 carry = make_int2(0, 0);
  for (int base = 0; base < ntiles; base += 256) {
    const int i = base + threadIdx.x;
    const int2 v = i < ntiles ? tiles[i] : make_int2(0, 0);
    int2 total;
    const int2 inc = selBlockScan(v, &total);
    if (i < ntiles) tiles[i] = make_int2(carry.x + inc.x - v.x, carry.y + inc.y - v.y);
    carry = selAdd(carry, total);
  }
  if (threadIdx.x == 0) {
    if (slot_x >= 0) counters[slot_x] = carry.x;
    if (slot_y >= 0) counters[slot_y] = carry.y;
  }
}
__global__ void __launch_bounds__(256) k_sel_scanB(int2* __restrict__ tiles, const int ntiles, int* __restrict__ counters, const int slot_x, const int slot_y) {
  selScanBBody(tiles, ntiles, counters, slot_x, slot_y);
}
// CELL: n2ex[i] (and n2ex[n]); NZ: rn[i]; SURV: clears the dropped entries, writes the compacted lists
template <int MODE> __device__ __forceinline__ void selScanCBody(const SelScanArgs& A, const unsigned int* __restrict__ mask, unsigned char* __restrict__ map,
                                                                 const int* __restrict__ rn, const unsigned char* __restrict__ pattern, const int2* __restrict__ tiles,
                                                                 int* __restrict__ out, int* __restrict__ lu, int* __restrict__ lv, int* __restrict__ lt,
                                                                 float* __restrict__ wu, float* __restrict__ wv) {
  const int base = blockIdx.x * SEL_TILE + threadIdx.x * 4;
  int2 v[4];
  int2 s = make_int2(0, 0);
#pragma unroll
  for (int k = 0; k < 4; k++) { v[k] = selScanVal<MODE>(A, mask, map, rn, pattern, base + k); s = selAdd(s, v[k]); }
  int2 total;
  const int2 inc = selBlockScan(s, &total);
  const int2 t0 = tiles[blockIdx.x];
  int2 ex = make_int2(t0.x + inc.x - s.x, t0.y + inc.y - s.y);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int i = base + k;
    if (i < A.n) {
      if (MODE == SEL_MODE_CELL) {
        out[i] = ex.x;
        if (i == A.n - 1) out[A.n] = ex.x + v[k].x;
      } else if (MODE == SEL_MODE_NZ) {
        out[i] = ex.x;
      } else {
        const unsigned char m = map[i];
        if (m != 0) {
          if (!v[k].x) map[i] = 0;   // :259
          else {
            const int x = i % A.w, y = i / A.w;
            lu[ex.x] = x; lv[ex.x] = y; lt[ex.x] = m;
            if (v[k].y) { wu[ex.y] = (float)x; wv[ex.y] = (float)y; }
          }
        }
      }
    }
    ex = selAdd(ex, v[k]);
  }
}
template <int MODE> __global__ void __launch_bounds__(256) k_sel_scanC(const SelScanArgs A, const unsigned int* __restrict__ mask, unsigned char* __restrict__ map,
                                                                        const int* __restrict__ rn, const unsigned char* __restrict__ pattern, const int2* __restrict__ tiles,
                                                                        int* __restrict__ out, int* __restrict__ lu, int* __restrict__ lv, int* __restrict__ lt,
                                                                        float* __restrict__ wu, float* __restrict__ wv) {
  selScanCBody<MODE>(A, mask, map, rn, pattern, tiles, out, lu, lv, lt, wu, wv);
}

// The recurrence itself, when a cell's selection depends on its direction: one wave, 64 cells per step, the next step's masks already in flight.  A group whose masks
// are all 0 / 0xFFFF advances by its popcount.  In a mixed group every lane tests its cell against the current direction; the first cell that selects ends the
// stretch (all cells up to it have their n2), n2 moves, the next direction comes out of a 128-entry window of randomPattern held in registers, and the rest of the group
// is tested again: one round per selection, none per cell.  Bounded by the cell count; waits on nothing.
__device__ __forceinline__ void selScanExactBody(const unsigned int* __restrict__ mask, const int ncell, const unsigned char* __restrict__ pattern, const int npattern,
                                                 int* __restrict__ n2ex, int* __restrict__ counters) {
  if (counters[SELC_MIXED] == 0) return;
  const int lane = threadIdx.x;
  int n2 = 0, wbase = 0;                                    // wave-uniform; window: lane j holds randomPattern[wbase + j] and [wbase + 64 + j]
  unsigned int w0 = pattern[lane], w1 = (64 + lane < npattern) ? pattern[64 + lane] : 0u;
  auto direction = [&]() -> int {
    while (n2 - wbase >= 64) {
      wbase += 64; w0 = w1;
      w1 = (wbase + 64 + lane < npattern) ? pattern[wbase + 64 + lane] : 0u;
    }
    return (int)(__builtin_amdgcn_readlane(w0, __builtin_amdgcn_readfirstlane(n2 - wbase)) & 15u);
  };
  int d = direction();
  // the masks of SEL_EXACT_AHEAD groups are loaded together, one chunk ahead of the one being walked: the walk itself never waits for memory
  unsigned int cur[SEL_EXACT_AHEAD], nxt[SEL_EXACT_AHEAD];
#pragma unroll
  for (int k = 0; k < SEL_EXACT_AHEAD; k++) cur[k] = (k * 64 + lane < ncell) ? mask[k * 64 + lane] : 0u;
  for (int base = 0; base < ncell; base += 64 * SEL_EXACT_AHEAD) {
#pragma unroll
    for (int k = 0; k < SEL_EXACT_AHEAD; k++) {
      const int j = base + 64 * SEL_EXACT_AHEAD + k * 64 + lane;
      nxt[k] = j < ncell ? mask[j] : 0u;
    }
#pragma unroll
    for (int k = 0; k < SEL_EXACT_AHEAD; k++) {
      const int i = base + k * 64 + lane;
      const unsigned int m = cur[k];
      int mine = n2;
      if (__ballot(m != 0u && m != 0xFFFFu) == 0ull) {
        const unsigned long long sel = __ballot(m != 0u);
        mine = n2 + __popcll(sel & ((1ull << lane) - 1ull));
        n2 += __popcll(sel);
        d = direction();
      } else {
        unsigned long long todo = ~0ull;
        while (todo) {
          const unsigned long long sel = __ballot(((m >> d) & 1u) != 0u) & todo;
          if ((todo >> lane) & 1ull) mine = n2;           // every cell up to and including the first that selects starts at this n2
          if (sel == 0ull) break;
          const int f = __builtin_ctzll(sel);
          todo = f == 63 ? 0ull : (todo & (~0ull << (f + 1)));
          n2++;
          d = direction();
        }
      }
      if (i < ncell) n2ex[i] = mine;
    }
#pragma unroll
    for (int k = 0; k < SEL_EXACT_AHEAD; k++) cur[k] = nxt[k];
  }
  if (lane == 0) { n2ex[ncell] = n2; counters[SELC_N2] = n2; counters[SELC_EXACT] = 1; }
}
__global__ void __launch_bounds__(64) k_sel_scan_exact(const unsigned int* __restrict__ mask, const int ncell, const unsigned char* __restrict__ pattern, const int npattern,
                                                       int* __restrict__ n2ex, int* __restrict__ counters) {
  selScanExactBody(mask, ncell, pattern, npattern, n2ex, counters);
}

// MAX of the keys of the lanes that share a target (id >= 0; lanes with the same id lie next to each other: a wave is 64 consecutive pixels of a row): a segmented
// scan, then one atomic per run instead of one per pixel
__device__ __forceinline__ void selRunMax(unsigned long long key, const int id, unsigned long long* __restrict__ base) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned int lo = (unsigned int)__shfl_up((int)(unsigned int)key, off, 64), hi = (unsigned int)__shfl_up((int)(unsigned int)(key >> 32), off, 64);
    const int oid = __shfl_up(id, off, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    if (lane >= off && oid == id && o > key) key = o;
  }
  const int nid = __shfl_down(id, 1, 64);
  if (id >= 0 && key != 0ull && (lane == 63 || nid != id)) selKeyMax(base + id, key);
}

// thread per pixel: its candidacies at the three levels.  keys = [key2: ncell | key3: ncell/4 | key4: ncell/16]
__device__ __forceinline__ void selPickBody(const float* __restrict__ I, const float* __restrict__ ag0, const float* __restrict__ ag1, const float* __restrict__ ag2,
                                            const float* __restrict__ thsS, const unsigned char* __restrict__ pattern, const int* __restrict__ n2ex, const SelGeom& G,
                                            unsigned long long* __restrict__ keys) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  // a pixel competes at level 0 (its cell selects) or at level 1 (its 2pot block holds no level-0 point), never both: one target; level 2 is a second one
  unsigned long long kA = 0ull, kB = 0ull;
  int idA = -1, idB = -1;
  const int x = idx % G.w, y = idx / G.w;
  if (idx < G.w * G.h && selInside(G, x, y)) {
    unsigned int rank;
    const int c = selCellOf(G, x, y, &rank);
    const unsigned int pp = (unsigned int)G.pot * (unsigned int)G.pot;
    const float pixelTH0 = thsS[(x >> 4) + (y >> 4) * G.nbW];
    const float pixelTH1 = pixelTH0 * G.dw1;
    const float pixelTH2 = pixelTH1 * G.dw2;
    const float2 g = gradAt(I, G.w, G.h, x, y);
    const int n2c = n2ex[c];
    const int c3 = c & ~3, c4 = c & ~15;
    if (n2ex[c + 1] != n2c) {
      // the cell selects: compete for it (:394-401); its 2pot / 4pot blocks hold a level-0 point
      const float a = ag0[idx];
      if (a > pixelTH0 * G.thFactor) {
        const float v = G.useDir ? selDirNorm(g, pattern[n2c] & 15) : a;
        if (v > 0.f) { kA = selKey(v, rank); idA = c; }
      }
    } else if (n2ex[c3 + 4] == n2ex[c3]) {
      const float a1 = ag1[(x >> 1) + (y >> 1) * G.w1];   // (int)(xf*0.5f+0.25f), :405
      if (a1 > pixelTH1 * G.thFactor) {
        const float v = G.useDir ? selDirNorm(g, pattern[n2c] & 15) : a1;   // n2 does not move inside such a block: n2 at its start = n2c
        if (v > 0.f) { kA = selKey(v, (unsigned int)(c & 3) * pp + rank); idA = G.ncell + (c >> 2); }
      }
      if (n2ex[c4 + 16] == n2ex[c4]) {
        const float a2 = ag2[(x >> 2) + (y >> 2) * G.w2];   // :417
        if (a2 > pixelTH2 * G.thFactor) {
          const float v = G.useDir ? selDirNorm(g, pattern[n2c] & 15) : a2;
          if (v > 0.f) { kB = selKey(v, (unsigned int)(c & 15) * pp + rank); idB = G.ncell + (G.ncell >> 2) + (c >> 4); }
        }
      }
    }
  }
  selRunMax(kA, idA, keys);
  if (__ballot(idB >= 0) != 0ull) selRunMax(kB, idB, keys);
}
__global__ void __launch_bounds__(256) k_sel_pick(const float* __restrict__ I, const float* __restrict__ ag0, const float* __restrict__ ag1, const float* __restrict__ ag2,
                                                  const float* __restrict__ thsS, const unsigned char* __restrict__ pattern, const int* __restrict__ n2ex, const SelGeom G,
                                                  unsigned long long* __restrict__ keys) {
  selPickBody(I, ag0, ag1, ag2, thsS, pattern, n2ex, G, keys);
}

// thread per cell: keys -> status map (:429-449), n3 / n4
__device__ __forceinline__ void selWriteBody(const int* __restrict__ n2ex, const unsigned long long* __restrict__ key2, const unsigned long long* __restrict__ key3,
                                             const unsigned long long* __restrict__ key4, const SelGeom& G, unsigned char* __restrict__ map, int* __restrict__ counters) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = c < G.ncell;
  const unsigned int pot = (unsigned int)G.pot, pp = pot * pot;
  const int n2c = live ? n2ex[c] : 0;
  bool hit3 = false, hit4 = false;
  if (live && n2ex[c + 1] != n2c) {
    const unsigned long long k = key2[c];
    if (k) {
      const unsigned int r = 0xFFFFFFFFu - (unsigned int)k;
      int x0, y0;
      selCellOrigin(G, c, &x0, &y0);
      map[(x0 + (int)(r % pot)) + (y0 + (int)(r / pot)) * G.w] = 1;
    }
  }
  if (live && (c & 3) == 0 && n2ex[c + 4] == n2c) {
    const unsigned long long k = key3[c >> 2];
    if (k) {
      const unsigned int r = 0xFFFFFFFFu - (unsigned int)k, q = r % pp;
      int x0, y0;
      selCellOrigin(G, c + (int)(r / pp), &x0, &y0);
      map[(x0 + (int)(q % pot)) + (y0 + (int)(q / pot)) * G.w] = 2;
      hit3 = true;
    }
  }
  if (live && (c & 15) == 0 && n2ex[c + 16] == n2c) {
    const int b3 = c >> 2;
    const unsigned long long k = key4[c >> 4];
    if (k && !key3[b3] && !key3[b3 + 1] && !key3[b3 + 2] && !key3[b3 + 3]) {
      const unsigned int r = 0xFFFFFFFFu - (unsigned int)k, q = r % pp;
      int x0, y0;
      selCellOrigin(G, c + (int)(r / pp), &x0, &y0);
      map[(x0 + (int)(q % pot)) + (y0 + (int)(q / pot)) * G.w] = 4;
      hit4 = true;
    }
  }
  // integer sums: per wave, then per workgroup through LDS, then one atomic per workgroup (atomics on one address are served one after the other: at potential 1
  // one per wave, 8000 of them, took 50 us)
  __shared__ int s_n[2];
  if (threadIdx.x < 2) s_n[threadIdx.x] = 0;
  __syncthreads();
  const int n3 = __popcll(__ballot(hit3)), n4 = __popcll(__ballot(hit4));
  if ((threadIdx.x & 63) == 0) {
    if (n3) atomicAdd(&s_n[0], n3);
    if (n4) atomicAdd(&s_n[1], n4);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_n[0]) atomicAdd(&counters[SELC_N3], s_n[0]);
    if (s_n[1]) atomicAdd(&counters[SELC_N4], s_n[1]);
  }
}
__global__ void __launch_bounds__(1024) k_sel_write(const int* __restrict__ n2ex, const unsigned long long* __restrict__ key2, const unsigned long long* __restrict__ key3,
                                                   const unsigned long long* __restrict__ key4, const SelGeom G, unsigned char* __restrict__ map, int* __restrict__ counters) {
  selWriteBody(n2ex, key2, key3, key4, G, map, counters);
}

}  // namespace dmv
