// Pixel selection for W keyframes per launch: the kernels of select_kernels.hpp with the window taken from the block index (the scheme of activate_batch_kernels.hpp).
// Every kernel here calls the body its single-window form calls (selAbsgradBody ... selWriteBody) on the arrays of ONE selector, so a window of a batch holds the bytes
// its single call would have left.
//   k_sel_absgrad_b, k_sel_hist_b, k_sel_smooth_b                  <- FrameHessian::makeImages' absSquaredGrad, PixelSelector::makeHists   (PixelSelector2.cpp:94-157)
//   k_sel_clear_b, k_sel_cellmask_b, k_sel_scanA/B/C_b<CELL>,
//   k_sel_scan_exact_b, k_sel_pick_b, k_sel_write_b                <- PixelSelector::select                                               (PixelSelector2.cpp:311-454)
//   k_sel_scanA/B/C_b<NZ | SURV>                                   <- the sub-selection of makeMaps (:247-265), the list of makeNewTraces (FullSystem.cpp:1653-1654)
// A round of the host's recursion (capi_select.hip) writes one slab of SelWin records and hands every kernel the slab.  Windows differ in potential, hence in cell
// count, scan tiles and k_sel_write grid: grid.x is the largest count of the batch, and a block past its own window's size, or a block of a window that takes no part in
// the phase, returns as a whole before its first barrier.  Whatever a workgroup loops on (the tile count, the cell count) comes from its own record and is the same for
// all its threads.  All atomics stay OR / MAX / integer ADD on the window's own arrays; no workgroup waits for another.
#pragma once
#include "select_kernels.hpp"

namespace dmv {

struct SelWin {
  const float *I0, *I1, *I2;        // the frame's levels 0..2
  const float* B;                   // the call's B table in the slab, or NULL
  float *ag, *ths, *thsS;
  const unsigned char* pattern;
  uint4* zero; int zero_words;      // the selector's scratch of this pass: [mask | key2 | key3 | key4 | map], in 16-byte words
  int* counters;                    // SELC_* of this window, in the batch's counter slab (one download per round)
  unsigned int* mask;
  unsigned long long* keys;         // key2 | key3 | key4 back to back
  unsigned char* map;
  int* n2ex; int2* tiles; int* rn;
  int *lu, *lv, *lt; float *wu, *wv;
  SelGeom G;
  SelScanArgs A;                    // of the phase: the cells of the pass, or the pixels of the final phase (charTH of the window's quotia)
  int h1, h2, nbH;                  // heights of levels 1 and 2 (their widths are G.w1, G.w2), thsSmoothed rows
  float histCut, histAdd;           // settings of the window's selector
  int active;                       // takes part in this round's select pass
  int sub;                          // final phase: takes the random sub-selection (quotia < 0.95)
};

// A pointer read from a record in memory is a generic pointer to the compiler and every access through it a flat_* instruction (activate_batch_kernels.hpp: actGl); read
// through an lvalue whose pointee type carries the global address space it stays a global one.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wincompatible-pointer-types-discards-qualifiers"
template <class T> __device__ __forceinline__ T* selGl(T* const& member) {
  return (T*)(*reinterpret_cast<__attribute__((address_space(1))) T* const*>(&member));
}
#pragma clang diagnostic pop

// does window V take part in a scan of MODE?  CELL: the round's select pass; NZ: the sub-selection; SURV: every window
__device__ __forceinline__ bool selScanOn(const SelWin& V, const int mode) { return mode == SEL_MODE_CELL ? V.active != 0 : (mode == SEL_MODE_NZ ? V.sub != 0 : true); }
__device__ __forceinline__ int selTilesOf(const SelWin& V) { return (V.A.n + SEL_TILE - 1) / SEL_TILE; }

// window = blockIdx.y (grid.x is the largest count of the batch) or, for the one-workgroup kernels, blockIdx.x
__global__ void __launch_bounds__(256) k_sel_clear_b(const SelWin* __restrict__ wins) {
  const SelWin& V = wins[blockIdx.y];
  if (!V.active) return;   // a window that has finished keeps its map
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < V.zero_words) selGl(V.zero)[i] = make_uint4(0u, 0u, 0u, 0u);
  if (i < SELC_COUNT) selGl(V.counters)[i] = 0;
}
__global__ void __launch_bounds__(256) k_sel_absgrad_b(const SelWin* __restrict__ wins) {
  const SelWin& V = wins[blockIdx.y];
  selAbsgradBody(selGl(V.I0), selGl(V.I1), selGl(V.I2), V.G.w, V.G.h, V.G.w1, V.h1, V.G.w2, V.h2, selGl(V.B), selGl(V.ag));
}
__global__ void __launch_bounds__(256) k_sel_hist_b(const SelWin* __restrict__ wins) {
  const SelWin& V = wins[blockIdx.y];
  selHistBody((const float*)selGl(V.ag), V.G.w, V.G.h, V.G.nbW, V.histCut, V.histAdd, selGl(V.ths));
}
__global__ void __launch_bounds__(256) k_sel_smooth_b(const SelWin* __restrict__ wins) {
  const SelWin& V = wins[blockIdx.y];
  selSmoothBody((const float*)selGl(V.ths), V.G.nbW, V.nbH, selGl(V.thsS));
}
__global__ void __launch_bounds__(256) k_sel_cellmask_b(const SelWin* __restrict__ wins) {
  const SelWin& V = wins[blockIdx.y];
  if (!V.active) return;
  selCellmaskBody(selGl(V.I0), (const float*)selGl(V.ag), (const float*)selGl(V.thsS), V.G, selGl(V.mask));
}
template <int MODE> __global__ void __launch_bounds__(256) k_sel_scanA_b(const SelWin* __restrict__ wins) {
  const SelWin& V = wins[blockIdx.y];
  if (!selScanOn(V, MODE) || (int)blockIdx.x >= selTilesOf(V)) return;
  selScanABody<MODE>(V.A, (const unsigned int*)selGl(V.mask), (const unsigned char*)selGl(V.map), (const int*)(MODE == SEL_MODE_SURV && V.sub ? selGl(V.rn) : nullptr),
                     selGl(V.pattern), selGl(V.tiles));
}
// one workgroup per window: loops over its own window's tile count
__global__ void __launch_bounds__(256) k_sel_scanB_b(const SelWin* __restrict__ wins, const int mode, const int slot_x, const int slot_y) {
  const SelWin& V = wins[blockIdx.x];
  if (!selScanOn(V, mode)) return;
  selScanBBody(selGl(V.tiles), selTilesOf(V), selGl(V.counters), slot_x, slot_y);
}
template <int MODE> __global__ void __launch_bounds__(256) k_sel_scanC_b(const SelWin* __restrict__ wins) {
  const SelWin& V = wins[blockIdx.y];
  if (!selScanOn(V, MODE) || (int)blockIdx.x >= selTilesOf(V)) return;
  selScanCBody<MODE>(V.A, (const unsigned int*)selGl(V.mask), selGl(V.map), (const int*)(MODE == SEL_MODE_SURV && V.sub ? selGl(V.rn) : nullptr), selGl(V.pattern),
                     (const int2*)selGl(V.tiles), MODE == SEL_MODE_CELL ? selGl(V.n2ex) : (MODE == SEL_MODE_NZ ? selGl(V.rn) : (int*)nullptr), selGl(V.lu), selGl(V.lv), selGl(V.lt), selGl(V.wu), selGl(V.wv));
}
// one wave per window; returns at once when its window has no mixed cell (selScanExactBody reads SELC_MIXED) or takes no part in the round
__global__ void __launch_bounds__(64) k_sel_scan_exact_b(const SelWin* __restrict__ wins) {
  const SelWin& V = wins[blockIdx.x];
  if (!V.active) return;
  selScanExactBody((const unsigned int*)selGl(V.mask), V.G.ncell, selGl(V.pattern), V.G.w * V.G.h, selGl(V.n2ex), selGl(V.counters));
}
__global__ void __launch_bounds__(256) k_sel_pick_b(const SelWin* __restrict__ wins) {
  const SelWin& V = wins[blockIdx.y];
  if (!V.active) return;
  const float* ag0 = selGl(V.ag);
  const float* ag1 = ag0 + V.G.w * V.G.h;
  const float* ag2 = ag1 + V.G.w1 * V.h1;
  selPickBody(selGl(V.I0), ag0, ag1, ag2, (const float*)selGl(V.thsS), selGl(V.pattern), (const int*)selGl(V.n2ex), V.G, selGl(V.keys));
}
__global__ void __launch_bounds__(1024) k_sel_write_b(const SelWin* __restrict__ wins) {
  const SelWin& V = wins[blockIdx.y];
  if (!V.active || (int)(blockIdx.x * blockDim.x) >= V.G.ncell) return;
  const unsigned long long* key2 = selGl(V.keys);
  selWriteBody((const int*)selGl(V.n2ex), key2, key2 + V.G.ncell, key2 + V.G.ncell + V.G.ncell / 4, V.G, selGl(V.map), selGl(V.counters));
}

}  // namespace dmv
