// CDNA4 (gfx950) kernels of the batched window hand-over (dmvio_hip_ba_set_graph_from_batch, ba_graph_batch_host.hpp): what dmvio_hip_ba_set_graph_from enqueues per
// window — the arena memsets, the 0xff fill of the residual table, two or three merged copies and the four k_ba_scd_* launches — for W windows in six launches.  The
// windows keep their own arenas: the host lays every handle's arrays out exactly as the single call does and describes, per window, the byte ranges to clear and the
// pieces of the uploaded slab to copy where.  No arithmetic: the arrays a window ends up with are the single call's, byte for byte.
// Every kernel takes its window from blockIdx.y through the window's record; the pointers a record or a table holds are read through gl() (ba_batch_kernels.hpp): a
// pointer loaded from memory is a generic pointer to the compiler, and every access through it a flat_* instruction.
#pragma once
#include "ba_batch_kernels.hpp"

namespace dmv {

// 16-byte units throughout: arena allocations and the slab's pieces start on 256-byte granules and own their padding
struct BAGraphRange { uint4* p; unsigned long long n16; unsigned int value, pad; };   // fill [p, p + n16) with `value` in every 32-bit word
struct BAGraphSeg { uint4* dst; const uint4* src; unsigned long long n16; };          // dst[0 .. n16) = src[0 .. n16)
enum { BA_GRAPH_MAX_SEGS = 20 };
struct BAGraphWinDev {
  int F, N, R;
  int n_ranges, n_segs, pad;
  const BAGraphRange* ranges;   // in the uploaded slab
  const BAGraphSeg* segs;
  // the Schur buckets' member lists (ba_kernels.hpp: k_ba_scd_*), in the handle's arena
  const int *point, *target, *host, *pt_first, *pt_last;
  int *ridx, *cnt, *scd_begin, *scd_members;
};

// the arena ranges the windows' previous graphs used, cleared; the residual table of the new graph set to -1 (the host cuts the table's range out of the cleared ones:
// no byte is written twice in a launch)
__global__ void __launch_bounds__(256) k_ba_graph_clear_b(const BAGraphWinDev* __restrict__ wins) {
  const BAGraphWinDev& V = wins[blockIdx.y];
  const BAGraphRange* const ranges = gl(V.ranges);
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  for (int r = 0; r < V.n_ranges; r++) {
    const BAGraphRange& g = ranges[r];
    uint4* const p = gl(g.p);
    const unsigned long long n16 = g.n16;
    const unsigned int v = g.value;
    const uint4 fill = make_uint4(v, v, v, v);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) p[i] = fill;
  }
}
// the uploaded tables into each handle's arena arrays
__global__ void __launch_bounds__(256) k_ba_graph_scatter_b(const BAGraphWinDev* __restrict__ wins) {
  const BAGraphWinDev& V = wins[blockIdx.y];
  const BAGraphSeg* const segs = gl(V.segs);
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  for (int k = 0; k < V.n_segs; k++) {
    const BAGraphSeg& g = segs[k];
    uint4* const dst = gl(g.dst);
    const uint4* const src = gl(g.src);
    const unsigned long long n16 = g.n16;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
  }
}
// k_ba_scd_ridx / _lists / _scan per window: F, N, R and the arrays from the record; grid.x is the largest window's
__global__ void __launch_bounds__(256) k_ba_scd_ridx_b(const BAGraphWinDev* __restrict__ wins) {
  const BAGraphWinDev& V = wins[blockIdx.y];
  baScdRidxBody(blockIdx.x * 256 + threadIdx.x, V.R, V.F, gl(V.point), gl(V.target), gl(V.ridx));
}
// grid.x = F x (F*F / 4 workgroups, rounded up) of the call's largest keyframe count: host keyframe h = blockIdx.x / (the window's own workgroups per keyframe)
__global__ void __launch_bounds__(256) k_ba_scd_lists_b(const BAGraphWinDev* __restrict__ wins, const int mode) {
  const BAGraphWinDev& V = wins[blockIdx.y];
  const int F = V.F, nb = (F * F + 3) / 4;
  const int h = blockIdx.x / nb;
  if (h >= F) return;
  baScdListsBody(h, blockIdx.x - h * nb, F, gl(V.pt_first), gl(V.pt_last), gl(V.host), gl(V.ridx), mode, gl(V.cnt), gl(V.scd_begin), gl(V.scd_members));
}
__global__ void __launch_bounds__(1024) k_ba_scd_scan_b(const BAGraphWinDev* __restrict__ wins) {
  __shared__ int s[2048];
  const BAGraphWinDev& V = wins[blockIdx.y];
  baScdScanBody(s, V.F * V.F * V.F, gl(V.cnt), gl(V.scd_begin));
}

}  // namespace dmv
