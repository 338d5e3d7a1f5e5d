// The 4 x 8 pixel block of the wave-autonomous pyramid builds: what a thread of k_build_pyramids_reg / k_build_pyramids_raw_reg (image_kernels.hpp) does for its block, in a
// header of its own because the batched tracking kernel that builds the pyramids of deferred attaches (k_track_lm_build, tracker_kernels.hpp) runs the same code in its
// prologue and the unit of that kernel does not compile the image kernels.
#pragma once
#include "common.h"

namespace dmv {

typedef float pyr_f4 __attribute__((ext_vector_type(4)));

// Levels 1..3 of a thread's 4 x 8 pixel block (k_build_pyramids_raw_reg, k_build_pyramids_reg): 2 x 4 values of level 1 and two of level 2 in registers, level 3 by the even
// lane of a lane pair.  0.25f * (((a + b) + c) + d) per level, the reference's operand order (HessianBlocks.cpp:150-166).
__device__ __forceinline__ void pyrRegCoarse(const float (&v)[8][4], const PyrGeom& G, const FrameStore& fs, const int slot, const int tx, const int ty, const bool live, const int lane) {
  if (G.levels < 2) return;
  float l1[4][2];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 2; c++) l1[r][c] = 0.25f * (v[2 * r][2 * c] + v[2 * r][2 * c + 1] + v[2 * r + 1][2 * c] + v[2 * r + 1][2 * c + 1]);
  if (live) {
    float* __restrict__ d1 = fs.own_level(slot, 1);
    const int w1 = G.w[1];
#pragma unroll
    for (int r = 0; r < 4; r++) { const float2 q = make_float2(l1[r][0], l1[r][1]); __builtin_memcpy(d1 + (size_t)(4 * ty + r) * w1 + 2 * tx, &q, 8); }
  }
  if (G.levels < 3) return;
  float l2[2];
#pragma unroll
  for (int r = 0; r < 2; r++) l2[r] = 0.25f * (l1[2 * r][0] + l1[2 * r][1] + l1[2 * r + 1][0] + l1[2 * r + 1][1]);
  if (live) {
    float* __restrict__ d2 = fs.own_level(slot, 2);
    const int w2 = G.w[2];
    d2[(size_t)(2 * ty) * w2 + tx] = l2[0];
    d2[(size_t)(2 * ty + 1) * w2 + tx] = l2[1];
  }
  if (G.levels < 4) return;
  // level 3: the 2 x 2 block of level 2 = this lane's two values and those of the lane to its right (w0 % 8 == 0: a lane pair never straddles a block row)
  const float nb0 = __shfl_down(l2[0], 1, 64), nb1 = __shfl_down(l2[1], 1, 64);
  if (live && !(lane & 1)) fs.own_level(slot, 3)[(size_t)ty * G.w[3] + (tx >> 1)] = 0.25f * (l2[0] + nb0 + l2[1] + nb1);
}

// One 4 x 8 block of the wave-autonomous build of fp32 images resident on the device (k_build_pyramids_reg below): block t of the frame at src (row-major, (w0 / 4) * (h0 / 8) blocks; t beyond them: a dead lane that computes on block 0 and stores nothing).
// The eight row loads, the |v| <= 1e30 test, the caller's stamps (`stamp(bad, live)`, between the test and the stores as in the kernel this was taken out of), level 0 unless
// ATTACH, and pyrRegCoarse.  Shared by k_build_pyramids_reg and by the prologue of k_track_lm_build (tracker_kernels.hpp), so the two write the same planes by construction.
// The lane pair of level 3 must be adjacent blocks: every caller hands consecutive t to consecutive lanes and keeps whole wavefronts in the call.
template <bool ATTACH, class Stamp>
__device__ __forceinline__ void pyrRegBlock(const float* __restrict__ src, const PyrGeom& G, const FrameStore& fs, const int slot, const int t, const int lane, Stamp&& stamp) {
  const int w0 = G.w[0], h0 = G.h[0];
  const int tpr4 = w0 >> 2, nthr = tpr4 * (h0 >> 3);
  const bool live = t < nthr;
  const int tx = live ? t % tpr4 : 0, ty = live ? t / tpr4 : 0;
  const int x = 4 * tx, y = 8 * ty;
  float v[8][4];
  const float* __restrict__ p0 = src + (size_t)y * w0 + x;
  if (((uintptr_t)src & 15) == 0) {   // x % 4 == 0, w0 % 8 == 0: the frame's base decides for every row
#pragma unroll
    for (int r = 0; r < 8; r++) { const pyr_f4 q = __builtin_nontemporal_load(reinterpret_cast<const pyr_f4*>(p0 + (size_t)r * w0)); v[r][0] = q[0]; v[r][1] = q[1]; v[r][2] = q[2]; v[r][3] = q[3]; }
  } else {
#pragma unroll
    for (int r = 0; r < 8; r++) __builtin_memcpy(v[r], p0 + (size_t)r * w0, 16);
  }
  bool bad = false;
#pragma unroll
  for (int r = 0; r < 8; r++)
#pragma unroll
    for (int k = 0; k < 4; k++) bad |= !(fabsf(v[r][k]) <= 1e30f);
  stamp(bad, live);
  if (!ATTACH && live) {
    float* __restrict__ dst0 = fs.own_level(slot, 0);
    if (((uintptr_t)dst0 & 15) == 0) {
#pragma unroll
      for (int r = 0; r < 8; r++) { const pyr_f4 q = {v[r][0], v[r][1], v[r][2], v[r][3]}; __builtin_nontemporal_store(q, reinterpret_cast<pyr_f4*>(dst0 + (size_t)(y + r) * w0 + x)); }
    } else {
#pragma unroll
      for (int r = 0; r < 8; r++) __builtin_memcpy(dst0 + (size_t)(y + r) * w0 + x, v[r], 16);
    }
  }
  pyrRegCoarse(v, G, fs, slot, tx, ty, live, lane);
}

}  // namespace dmv
