// The per-point passes of CoarseInitializer::trackFrame (src/dso/FullSystem/CoarseInitializer.cpp) on a point set that lives on the device: resetPoints, doStep, applyStep,
// calcEC, optReg, propagateUp, propagateDown and the unsnapped reset.  Every per-point value has the reference's bits: the same single-precision operations in the same
// order, no contraction (the unit is compiled with -ffp-contract=off, like the reference).  Every pointer is a kernel argument, so every access is a global_* one.
#pragma once
#include "common.h"

namespace dmv {

struct InitInc8 { float v[8]; };

// trackFrame's reset while the initializer has not snapped (:100-114)
__device__ __forceinline__ void initResetUnsnappedPoint(const int i, float* __restrict__ iR, float* __restrict__ idepth_new, float* __restrict__ lastHessian) {
  iR[i] = 1.0f; idepth_new[i] = 1.0f; lastHessian[i] = 0.0f;
}
inline __global__ void __launch_bounds__(256) k_init_reset_unsnapped(const int n, float* __restrict__ iR, float* __restrict__ idepth_new, float* __restrict__ lastHessian) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  initResetUnsnappedPoint(i, iR, idepth_new, lastHessian);
}

// The per-point bodies (initResetUnsnappedPoint, initResetPoint, initDoStepPoint, initApplyStepPoint, initPropagateUpPoint, initPropagateDownPoint) are shared with the
// device-resident LM loop (init_lm_kernels.hpp: k_init_lm; init_lm_batch_kernels.hpp: k_init_lm_frame_b), which runs them for the same i from one workgroup.

// resetPoints, the part every level takes (:895-898)
__device__ __forceinline__ void initResetPoint(const int i, const float* __restrict__ idepth, float* __restrict__ idepth_new, float* __restrict__ energy /* 2n */) {
  energy[2 * i] = 0.0f; energy[2 * i + 1] = 0.0f;
  idepth_new[i] = idepth[i];
}
inline __global__ void __launch_bounds__(256) k_init_reset_points(const int n, const float* __restrict__ idepth, float* __restrict__ idepth_new, float* __restrict__ energy /* 2n */) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  initResetPoint(i, idepth, idepth_new, energy);
}

// doStep (:919-947).  The 8-term dot is summed in index order, then added to Jb[8]: the order the compiled reference's Eigen stand-in takes.
__device__ __forceinline__ void initDoStepPoint(const int i, const float lambda, const InitInc8& inc, const unsigned char* __restrict__ isGood,
                                                const float* __restrict__ Jb /* 10n */, const float* __restrict__ maxstep_in, const float* __restrict__ idepth,
                                                float* __restrict__ idepth_new) {
  if (!isGood[i]) return;
  const float* __restrict__ J = Jb + 10 * (size_t)i;
  float s = J[0] * inc.v[0];
#pragma unroll
  for (int k = 1; k < 8; k++) s += J[k] * inc.v[k];
  const float b = J[8] + s;
  float step = -b * J[9] / (1 + lambda);
  float maxstep = 0.25f * maxstep_in[i];
  if (maxstep > 1e10f) maxstep = 1e10f;
  if (step > maxstep) step = maxstep;
  if (step < -maxstep) step = -maxstep;
  float newIdepth = idepth[i] + step;
  if (newIdepth < 1e-3) newIdepth = 1e-3;   // (double comparisons and a rounded constant, as written there)
  if (newIdepth > 50) newIdepth = 50;
  idepth_new[i] = newIdepth;
}
inline __global__ void __launch_bounds__(256) k_init_do_step(const int n, const float lambda, const InitInc8 inc, const unsigned char* __restrict__ isGood,
                                                      const float* __restrict__ Jb /* 10n */, const float* __restrict__ maxstep_in, const float* __restrict__ idepth,
                                                      float* __restrict__ idepth_new) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  initDoStepPoint(i, lambda, inc, isGood, Jb, maxstep_in, idepth, idepth_new);
}

// applyStep (:948-963); the swap of the two JbBuffers (:964) is a pointer swap in the handle
__device__ __forceinline__ void initApplyStepPoint(const int i, unsigned char* __restrict__ isGood, const unsigned char* __restrict__ isGood_new,
                                                   float* __restrict__ idepth, float* __restrict__ idepth_new, const float* __restrict__ iR,
                                                   float* __restrict__ energy, const float* __restrict__ energy_new, float* __restrict__ lastHessian,
                                                   const float* __restrict__ lastHessian_new) {
  if (!isGood[i]) { const float r = iR[i]; idepth[i] = r; idepth_new[i] = r; return; }
  energy[2 * i] = energy_new[2 * i]; energy[2 * i + 1] = energy_new[2 * i + 1];
  isGood[i] = isGood_new[i];
  idepth[i] = idepth_new[i];
  lastHessian[i] = lastHessian_new[i];
}
inline __global__ void __launch_bounds__(256) k_init_apply_step(const int n, unsigned char* __restrict__ isGood, const unsigned char* __restrict__ isGood_new,
                                                         float* __restrict__ idepth, float* __restrict__ idepth_new, const float* __restrict__ iR,
                                                         float* __restrict__ energy, const float* __restrict__ energy_new, float* __restrict__ lastHessian,
                                                         const float* __restrict__ lastHessian_new) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  initApplyStepPoint(i, isGood, isGood_new, idepth, idepth_new, iR, energy, energy_new, lastHessian, lastHessian_new);
}

// ---- the ordered sweeps.  ONE workgroup of one wavefront walks the levels of the static schedule (init_resident_host.hpp); iR and isGood of the whole point set live in
// LDS for the walk (5 n bytes, dynamic) and go back at the end.  A level's points are independent of one another, so a level wider than the wavefront is taken in chunks
// without a barrier between them; between two levels there is one.
struct InitSweepOptReg {   // optReg's body (:683-701)
  float regWeight;
  const float* __restrict__ idepth;
  __device__ __forceinline__ void operator()(const int i, const int* __restrict__ nb, float* __restrict__ s_iR, unsigned char* __restrict__ s_good) const {
    if (!s_good[i]) return;
    float idnn[10];
    int nnn = 0;
#pragma unroll
    for (int j = 0; j < 10; j++) {
      const int o = nb[j];
      const int oo = o < 0 ? 0 : o;   // (i exists, so entry 0 does)
      const bool take = o != -1 && s_good[oo];
      idnn[j] = take ? s_iR[oo] : __builtin_inff();
      nnn += take ? 1 : 0;
    }
    if (nnn > 2) {
      // sorted[nnn / 2] of the taken values (what std::nth_element leaves at that position): the value with `less` <= nnn/2 < `less` + `equal`; the entries not taken
      // are +inf and sort behind every taken one
      const int m = nnn / 2;
      float med = 0.0f;
#pragma unroll
      for (int a = 0; a < 10; a++) {
        int less = 0, eq = 0;
#pragma unroll
        for (int b = 0; b < 10; b++) { less += idnn[b] < idnn[a] ? 1 : 0; eq += idnn[b] == idnn[a] ? 1 : 0; }
        if (less <= m && m < less + eq) med = idnn[a];
      }
      s_iR[i] = (1 - regWeight) * idepth[i] + regWeight * med;
    }
  }
};
struct InitSweepResetTop {   // resetPoints on the top level: a point that is not good takes the mean iR of its good neighbours (:901-916)
  float* __restrict__ idepth;
  float* __restrict__ idepth_new;
  __device__ __forceinline__ void operator()(const int i, const int* __restrict__ nb, float* __restrict__ s_iR, unsigned char* __restrict__ s_good) const {
    if (s_good[i]) return;
    float snd = 0, sn = 0;
#pragma unroll
    for (int j = 0; j < 10; j++) {
      const int o = nb[j];
      if (o == -1 || !s_good[o]) continue;
      snd += s_iR[o];
      sn += 1;
    }
    if (sn > 0) {
      const float r = snd / sn;
      s_good[i] = 1;
      s_iR[i] = r; idepth[i] = r; idepth_new[i] = r;
    }
  }
};

template <class BODY>
inline __global__ void __launch_bounds__(64) k_init_sweep(const int n, const int levels, const int* __restrict__ level_begin, const int* __restrict__ order,
                                                   const int* __restrict__ neighbours /* 10n */, float* __restrict__ iR, unsigned char* __restrict__ isGood, const BODY body) {
  extern __shared__ float s_sweep[];
  float* __restrict__ s_iR = s_sweep;
  unsigned char* __restrict__ s_good = reinterpret_cast<unsigned char*>(s_sweep + n);
  const int t = threadIdx.x;
  for (int i = t; i < n; i += 64) { s_iR[i] = iR[i]; s_good[i] = isGood[i]; }
  __syncthreads();
  int begin = levels > 0 ? level_begin[0] : 0;
  for (int l = 0; l < levels; l++) {
    const int end = level_begin[l + 1];
    for (int k = begin + t; k < end; k += 64) {
      const int i = order[k];
      int nb[10];
#pragma unroll
      for (int j = 0; j < 10; j++) nb[j] = neighbours[10 * (size_t)i + j];
      body(i, nb, s_iR, s_good);
    }
    __syncthreads();
    begin = end;
  }
  for (int i = t; i < n; i += 64) { iR[i] = s_iR[i]; isGood[i] = s_good[i]; }
}

// propagateUp (:713-744): one thread per parent walks its children in ascending index, as the reference's loop over the lower level meets them.
// n_listed: the parents child_begin covers (1 + the largest parent index of the lower level); a parent beyond has no child.
__device__ __forceinline__ void initPropagateUpPoint(const int p, const int n_listed, const int* __restrict__ child_begin, const int* __restrict__ children,
                                                     const unsigned char* __restrict__ src_good, const float* __restrict__ src_iR, const float* __restrict__ src_lastHessian,
                                                     float* __restrict__ iR, float* __restrict__ idepth, unsigned char* __restrict__ isGood) {
  float acc = 0, num = 0;
  if (p < n_listed) {
    const int e = child_begin[p + 1];
    for (int k = child_begin[p]; k < e; k++) {
      const int c = children[k];
      if (!src_good[c]) continue;
      const float h = src_lastHessian[c];
      acc += src_iR[c] * h;
      num += h;
    }
  }
  if (num > 0) {
    const float r = acc / num;
    idepth[p] = r; iR[p] = r;
    isGood[p] = 1;
  } else {
    iR[p] = acc;   // the sum as far as it got: 0 for a parent without good children
  }
}
inline __global__ void __launch_bounds__(256) k_init_propagate_up(const int n_dst, const int n_listed, const int* __restrict__ child_begin, const int* __restrict__ children,
                                                           const unsigned char* __restrict__ src_good, const float* __restrict__ src_iR, const float* __restrict__ src_lastHessian,
                                                           float* __restrict__ iR, float* __restrict__ idepth, unsigned char* __restrict__ isGood) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_dst) return;
  initPropagateUpPoint(p, n_listed, child_begin, children, src_good, src_iR, src_lastHessian, iR, idepth, isGood);
}

// propagateDown (:758-775): one thread per point of the lower level
__device__ __forceinline__ void initPropagateDownPoint(const int i, const int* __restrict__ parent, const unsigned char* __restrict__ par_good,
                                                       const float* __restrict__ par_iR, const float* __restrict__ par_lastHessian, unsigned char* __restrict__ isGood,
                                                       float* __restrict__ iR, float* __restrict__ idepth, float* __restrict__ idepth_new, float* __restrict__ lastHessian) {
  const int p = parent[i];
  const float ph = par_lastHessian[p];
  if (!par_good[p] || ph < 0.1) return;
  if (!isGood[i]) {
    const float r = par_iR[p];
    iR[i] = r; idepth[i] = r; idepth_new[i] = r;
    isGood[i] = 1;
    lastHessian[i] = 0;
  } else {
    const float lh = lastHessian[i];
    const float newiR = (iR[i] * lh * 2 + par_iR[p] * ph) / (lh * 2 + ph);
    iR[i] = newiR; idepth[i] = newiR; idepth_new[i] = newiR;
  }
}
inline __global__ void __launch_bounds__(256) k_init_propagate_down(const int n, const int* __restrict__ parent, const unsigned char* __restrict__ par_good,
                                                             const float* __restrict__ par_iR, const float* __restrict__ par_lastHessian, unsigned char* __restrict__ isGood,
                                                             float* __restrict__ iR, float* __restrict__ idepth, float* __restrict__ idepth_new, float* __restrict__ lastHessian) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  initPropagateDownPoint(i, parent, par_good, par_iR, par_lastHessian, isGood, iR, idepth, idepth_new, lastHessian);
}

// calcEC (:650-670): (sum rOld^2, sum rNew^2, count) over the points the evaluation accepted, in a fixed shape.  k_init_ec: initGrid(n) workgroups of 256, every thread
// adds its grid-stride points in index order, a wavefront folds with the xor butterfly (6 steps), the four wavefronts are added in order.  k_init_ec_final: one wavefront,
// lane l adds the partials l, l + 64, l + 128, l + 192 in order, then the same butterfly.  A term therefore passes through at most (k - 1) + 6 + 3 + 3 + 6 additions,
// k = ceil(n / (G * 256)) — tests/test_init_resident_gpu.py derives its bound from that.  The count is a sum of ones, exact below 2^24.
enum { IN_EC = 4 };   // floats per partial: rOld^2, rNew^2, count, pad
__device__ __forceinline__ float initWaveSum(float x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
// workgroup bx of the G (of 256 threads) that serve the point set; shared with k_init_lm, which runs bx = 0 .. G - 1 one after the other
__device__ __forceinline__ void initEcPartialBody(const int n, const unsigned char* __restrict__ isGood_new, const float* __restrict__ idepth, const float* __restrict__ idepth_new,
                                                  const float* __restrict__ iR, float* __restrict__ partials /* G x IN_EC */, const int bx, const int G) {
  __shared__ float s_part[4][3];
  float a = 0, b = 0, c = 0;
  for (int i = bx * 256 + threadIdx.x; i < n; i += G * 256) {
    if (!isGood_new[i]) continue;
    const float r = iR[i];
    const float rOld = idepth[i] - r, rNew = idepth_new[i] - r;
    a += rOld * rOld; b += rNew * rNew; c += 1.0f;
  }
  a = initWaveSum(a); b = initWaveSum(b); c = initWaveSum(c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_part[wave][0] = a; s_part[wave][1] = b; s_part[wave][2] = c; }
  __syncthreads();
  if (threadIdx.x < 3) {
    float s = s_part[0][threadIdx.x];
    for (int w = 1; w < 4; w++) s += s_part[w][threadIdx.x];
    partials[bx * IN_EC + threadIdx.x] = s;
  }
}
inline __global__ void __launch_bounds__(256) k_init_ec(const int n, const unsigned char* __restrict__ isGood_new, const float* __restrict__ idepth, const float* __restrict__ idepth_new,
                                                 const float* __restrict__ iR, float* __restrict__ partials /* gridDim.x x IN_EC */) {
  initEcPartialBody(n, isGood_new, idepth, idepth_new, iR, partials, blockIdx.x, gridDim.x);
}
// one wavefront (threadIdx.x < 64 of the caller); lane 0 stores
__device__ __forceinline__ void initEcFinalBody(const int G, const float* __restrict__ partials, float* __restrict__ out3) {
  float s[3] = {0, 0, 0};
  bool first = true;
  for (int g = threadIdx.x; g < G; g += 64) {
#pragma unroll
    for (int k = 0; k < 3; k++) s[k] = first ? partials[g * IN_EC + k] : s[k] + partials[g * IN_EC + k];
    first = false;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) s[k] = initWaveSum(s[k]);
  if (threadIdx.x == 0) { out3[0] = s[0]; out3[1] = s[1]; out3[2] = s[2]; }
}
inline __global__ void __launch_bounds__(64) k_init_ec_final(const int G, const float* __restrict__ partials, float* __restrict__ out3) {
  initEcFinalBody(G, partials, out3);
}

// good points whose pattern would leave the level (the evaluation reads (u + dx, v + dy), dx, dy in [-2, 2], and one pixel right / below, without a test): the count the
// resident evaluation's range check is made from where the host copy of (u, v) holds such a point at all
inline __global__ void __launch_bounds__(256) k_init_count_outside(const int n, const unsigned char* __restrict__ isGood, const float* __restrict__ u, const float* __restrict__ v,
                                                            const float umax, const float vmax, int* __restrict__ count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool out = i < n && isGood[i] && !(u[i] >= 2.0f && u[i] < umax && v[i] >= 2.0f && v[i] < vmax);
  const unsigned long long m = __ballot(out);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, __popcll(m));
}

// The point set setFirst makes (CoarseInitializer.cpp:841-865), adopted from lists that already live on the device (dmvio_hip_initializer_set_first): u, v, the
// neighbour table and the parents (parent_in NULL: the top level) are copied, idepth = iR = idepth_new = 1, isGood = 1, outlierTH the caller's constant.  Every other
// dynamic field has been cleared by the caller.
inline __global__ void __launch_bounds__(256) k_init_adopt(const int n, const float* __restrict__ u_in, const float* __restrict__ v_in, const int* __restrict__ nb_in,
                                                           const int* __restrict__ parent_in, const float outlierTH, float* __restrict__ u, float* __restrict__ v,
                                                           float* __restrict__ oth, int* __restrict__ nb, int* __restrict__ parent, float* __restrict__ idepth,
                                                           float* __restrict__ iR, float* __restrict__ idepth_new, unsigned char* __restrict__ isGood) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  u[i] = u_in[i]; v[i] = v_in[i]; oth[i] = outlierTH;
#pragma unroll
  for (int k = 0; k < 10; k++) nb[10 * (size_t)i + k] = nb_in[10 * (size_t)i + k];
  if (parent_in) parent[i] = parent_in[i];
  idepth[i] = 1.0f; iR[i] = 1.0f; idepth_new[i] = 1.0f; isGood[i] = 1;
}

}  // namespace dmv
