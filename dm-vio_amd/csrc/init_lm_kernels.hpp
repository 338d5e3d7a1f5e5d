// CoarseInitializer::trackFrame's Levenberg-Marquardt loop (src/dso/FullSystem/CoarseInitializer.cpp:126-255) on the device: ONE workgroup runs one level of one problem
// from resetPoints to the quit rule — control step (the 6x6 / 8x8 LDLT, SE3::exp, the affine update), doStep, the evaluation, calcEC, the accept test, applyStep, optReg
// and the lambda / fails / quit rules — without the host in between.  The per-point work is the resident unit's (init_resident_kernels.hpp) and the evaluation's
// (init_kernels.hpp) own device bodies, run by this workgroup for the virtual workgroups bx = 0 .. G - 1 of the host-driven calls one after the other: the partition of the
// points, the order inside every partial and the order of the final sums are theirs, so every per-point value, the 91 sums and the three calcEC sums have the bits of
// dmvio_hip_initializer_resident_calc at the same pose.  Compiled with -ffp-contract=off like those units.
#pragma once
#include "common.h"
#include "lie_dev.h"
#include "init_types.hpp"
#include "init_tail.hpp"
#include "init_kernels.hpp"
#include "init_resident_kernels.hpp"

namespace dmv {

enum { INIT_LM_MAX_ITER = 64, INIT_LM_TRACE_D = 20, INIT_LM_TRACE_F = 176 };

// ------------------------------------------------------------------------------------------------ the control step (:159-185), host and device
struct InitLmWs { float m[64], d[8], temp[8]; int tr[8]; };   // what the solve indexes dynamically: a device caller keeps it in LDS

// Hl = H with its diagonal times (1 + lambda), minus Hsc / (1 + lambda); bl = b - bsc / (1 + lambda); both scaled by wM and 0.01 / (w * h); inc = -wM * Hl^-1 bl by the
// pivoted LDLT (the 6x6 head with a zero tail when fix_affine); |inc|; SE3::exp(inc[0..5]) * refToNew; aff + inc[6..7].  Float operations in the order the compiled
// reference takes them: a trackFrame stepped by this function on the host reproduces the reference's own bit for bit (tests/golden/init_lm_frames.npz, both branches);
// the pose algebra as everywhere in this library (lie_dev.h).
DMV_HD void initLmControl(const float* H64, const float* b8, const float* Hsc64, const float* bsc8, const float lambda, const int wh, const float* wM8, const int fix_affine,
                          const double* pose7, const double* aff_ab, InitLmWs& ws, float* inc8, double* incNorm, double* pose7_new, double* aff_ab_new) {
  const float l1 = 1 + lambda;
  const float il = 1 / l1;
  const float sc = 0.01f / (float)wh;
  for (int i = 0; i < 8; i++) {
    for (int j = 0; j < 8; j++) {
      float h = H64[i * 8 + j];
      if (i == j) h *= l1;
      h = h - Hsc64[i * 8 + j] * il;
      ws.m[i * 8 + j] = ((wM8[i] * h) * wM8[j]) * sc;
    }
    const float bl = b8[i] - bsc8[i] * il;
    ws.d[i] = (wM8[i] * bl) * sc;
  }
  if (fix_affine) {
    ldltSolveInPlaceWs(ws.m, 8, ws.d, 6, ws.tr, ws.temp);
    // -(wM.toDenseMatrix().topLeftCorner<6, 6>() * x): a dense product, zeros included
    for (int i = 0; i < 6; i++) {
      float s = (i == 0 ? wM8[0] : 0.0f) * ws.d[0];
      for (int k = 1; k < 6; k++) s += (i == k ? wM8[i] : 0.0f) * ws.d[k];
      inc8[i] = -s;
    }
    inc8[6] = 0.0f; inc8[7] = 0.0f;
  } else {
    ldltSolveInPlaceWs(ws.m, 8, ws.d, 8, ws.tr, ws.temp);
    for (int i = 0; i < 8; i++) inc8[i] = -(wM8[i] * ws.d[i]);
  }
  float sq = inc8[0] * inc8[0];
  for (int i = 1; i < 8; i++) sq += inc8[i] * inc8[i];
  *incNorm = (double)sqrtf(sq);
  double a[6];
  for (int i = 0; i < 6; i++) a[i] = (double)inc8[i];
  poseTo7(poseMul(poseExp(a), poseFrom7(pose7)), pose7_new);
  aff_ab_new[0] = aff_ab[0] + inc8[6];
  aff_ab_new[1] = aff_ab[1] + inc8[7];
}

// the lambda / fails / quit rules behind the accept test (:216-250).  Returns whether the loop quits.
DMV_HD bool initLmRule(const bool accept, const double incNorm, const int iteration, const int max_iterations, float* lambda, int* fails) {
  if (accept) {
    *lambda *= 0.5;
    *fails = 0;
    if (*lambda < 0.0001) *lambda = 0.0001;
  } else {
    (*fails)++;
    *lambda *= 4;
    if (*lambda > 10000) *lambda = 10000;
  }
  const float eps = 1e-4;
  return !(incNorm > eps) || iteration >= max_iterations || *fails >= 2;
}

// ------------------------------------------------------------------------------------------------ records in device memory
struct InitLmState { double pose7[7], aff[2]; int snapped, pad; };   // refToNew, refToNew_aff, snapped: the context's record, carried from level to level and frame to frame
struct InitLmOut { float res3[3]; int iterations, tests, pad[3]; };   // per problem: resOld when the loop quit, the iteration it quit in, the accept tests made
struct InitLmTraceRec { double d[INIT_LM_TRACE_D]; float f[INIT_LM_TRACE_F]; };   // one per accept test; the indices: include/dmvio_hip_init_lm.h
// One problem = one level of one frame.  Addressed with blockIdx.x, so its members are wave-uniform scalar loads; its pointers are read through initGl().
struct InitLmProb {
  const float *Iref, *Inew, *u, *v, *outlierTH;
  float *idepth, *idepth_new, *iR, *energy, *energy_new, *maxstep, *lastHessian, *lastHessian_new, *jb[2];   // jb[cur] is JbBuffer, the other JbBuffer_new
  unsigned char *isGood, *isGood_new;
  const int *level_begin, *order, *neighbours;   // the static schedule of the ordered sweeps
  float *partials, *ecpartials;                  // G x IN_PART and G x IN_EC
  double Ki9[9], priorY, priorX;
  float fxfycxcy[4], wM8[8], alphaW, alphaK, regWeight, couplingWeight;
  int n, G, sweep_levels, cur, wl, hl, lvl, is_top_level, fix_affine, max_iterations, out_index, trace_base;
};

// ------------------------------------------------------------------------------------------------ the ordered sweeps, one wavefront
// k_init_sweep's walk (init_resident_kernels.hpp) with the loads of a level taken off its critical path: `order` and the ten neighbours of the first 64 points of level
// l + 1 are in registers before level l's bodies run, and between two levels stands a wavefront barrier, not a workgroup one (LDS operations of ONE wavefront execute in
// order).  The schedule only says which points are independent; every point sees the state its levels before left, as in the serial loop.  lane: 0 .. 63.
template <class BODY>
__device__ __forceinline__ void initLmSweepWalk(const int lane, const int levels, const int* __restrict__ level_begin, const int* __restrict__ order,
                                                const int* __restrict__ neighbours, float* __restrict__ s_iR, unsigned char* __restrict__ s_good, const BODY& body) {
  if (levels <= 0) return;
  int begin = level_begin[0], end = level_begin[1];
  int i_cur = -1, nb_cur[10];
#pragma unroll
  for (int j = 0; j < 10; j++) nb_cur[j] = -1;
  if (begin + lane < end) {
    i_cur = order[begin + lane];
#pragma unroll
    for (int j = 0; j < 10; j++) nb_cur[j] = neighbours[10 * (size_t)i_cur + j];
  }
  for (int l = 0; l < levels; l++) {
    const int nend = l + 1 < levels ? level_begin[l + 2] : end;
    int i_nxt = -1, nb_nxt[10];
#pragma unroll
    for (int j = 0; j < 10; j++) nb_nxt[j] = -1;
    if (l + 1 < levels && end + lane < nend) {
      i_nxt = order[end + lane];
#pragma unroll
      for (int j = 0; j < 10; j++) nb_nxt[j] = neighbours[10 * (size_t)i_nxt + j];
    }
    if (i_cur >= 0) body(i_cur, nb_cur, s_iR, s_good);
    for (int k = begin + 64 + lane; k < end; k += 64) {   // a level wider than the wavefront: its points are independent of one another
      const int i = order[k];
      int nb[10];
#pragma unroll
      for (int j = 0; j < 10; j++) nb[j] = neighbours[10 * (size_t)i + j];
      body(i, nb, s_iR, s_good);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    begin = end; end = nend; i_cur = i_nxt;
#pragma unroll
    for (int j = 0; j < 10; j++) nb_cur[j] = nb_nxt[j];
  }
}
// the whole sweep by a workgroup of T threads: iR and isGood into LDS, the walk by wavefront 0, and back
template <int T, class BODY>
__device__ __forceinline__ void initLmSweep(const int n, const int levels, const int* __restrict__ level_begin, const int* __restrict__ order, const int* __restrict__ neighbours,
                                            float* __restrict__ iR, unsigned char* __restrict__ isGood, float* __restrict__ s_iR, unsigned char* __restrict__ s_good,
                                            const BODY& body) {
  const int t = threadIdx.x;
  __syncthreads();   // what the passes before wrote is visible
  for (int i = t; i < n; i += T) { s_iR[i] = iR[i]; s_good[i] = isGood[i]; }
  __syncthreads();
  if (t < 64) initLmSweepWalk(t, levels, level_begin, order, neighbours, s_iR, s_good, body);
  __syncthreads();
  for (int i = t; i < n; i += T) { iR[i] = s_iR[i]; isGood[i] = s_good[i]; }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------ k_init_lm
struct InitLmSys { float H[64], b[8], Hsc[64], bsc[8], res3[3], pad; };
struct InitLmCtl {
  double pose[7], aff[2], pose_new[7], aff_new[2], incNorm;
  float inc[8], ec3[3], tlog[3], lambda, lambda_used, eOld, eNew;
  int snapped, fails, it, quit, accept, cur_sys, tests, pad;
};

// the LDS blocks of one level's loop, beside the sweeps' dynamic 5 n bytes
struct InitLmLds {
  InitLmSys sys[2];
  float sums[IN_PART], ecsum[4];
  InitArgs A;
  InitLmWs ws;
  InitLmCtl c;
};

// One level of one problem by the 256 threads of the calling workgroup, from the state record to the state record: the body of k_init_lm, and of every level k_init_lm_frame_b
// (init_lm_batch_kernels.hpp) walks.  Every thread of the workgroup calls it; it ends with the record, the level's out and its trace records written by lane 0 — a caller that
// goes on in the same launch puts a workgroup barrier behind it.
__device__ __forceinline__ void initLmLevel(const InitLmProb& V, InitLmState* __restrict__ state, InitLmOut* __restrict__ outs, InitLmTraceRec* __restrict__ trace,
                                            float* __restrict__ s_sweep, InitLmLds& S) {
  InitLmSys* const s_sys = S.sys;
  float* const s_sums = S.sums;
  float* const s_ecsum = S.ecsum;
  InitArgs& s_A = S.A;
  InitLmWs& s_ws = S.ws;
  InitLmCtl& s_c = S.c;
  const int t = threadIdx.x, n = V.n, G = V.G;
  const float *Iref = initGl(V.Iref), *Inew = initGl(V.Inew), *u = initGl(V.u), *v = initGl(V.v), *outlierTH = initGl(V.outlierTH);
  float *idepth = initGl(V.idepth), *idepth_new = initGl(V.idepth_new), *iR = initGl(V.iR), *energy = initGl(V.energy), *energy_new = initGl(V.energy_new);
  float *maxstep = initGl(V.maxstep), *lastHessian = initGl(V.lastHessian), *lastHessian_new = initGl(V.lastHessian_new);
  float *jb0 = initGl(V.jb[0]), *jb1 = initGl(V.jb[1]);
  unsigned char *isGood = initGl(V.isGood), *isGood_new = initGl(V.isGood_new);
  const int *level_begin = initGl(V.level_begin), *order = initGl(V.order), *neighbours = initGl(V.neighbours);
  float *partials = initGl(V.partials), *ecpartials = initGl(V.ecpartials);
  float* s_iR = s_sweep;
  unsigned char* s_good = reinterpret_cast<unsigned char*>(s_sweep + n);
  int cur = V.cur;

  // the uniform inputs of an evaluation at (pose7, aff), by lane 0
  auto makeArgs = [&](const double* pose7, const double* aff) __attribute__((always_inline)) {
    s_A = initMakeArgsAt(V.wl, V.hl, V.Ki9, V.fxfycxcy, poseFrom7(pose7), aff, n, V.alphaW, V.alphaK, V.couplingWeight);
  };
  // calcResAndGS up to the 91 sums: the G virtual workgroups of the host-driven call one after the other, then k_init_final's sum in index order
  auto evaluate = [&]() __attribute__((always_inline)) {
    const InitArgs A = s_A;
    InitPts P;
    P.n = n; P.u = u; P.v = v; P.idepth_new = idepth_new; P.iR = iR; P.energy = energy; P.outlierTH = outlierTH; P.isGood = isGood;
    P.energy_new = energy_new; P.maxstep = maxstep; P.lastHessian_new = lastHessian_new; P.JbBuffer_new = cur ? jb0 : jb1; P.isGood_new = isGood_new;
    for (int bx = 0; bx < G; bx++) initPartialBody(Iref, Inew, P, A, partials, bx, G);
    __syncthreads();
    if (t < IN_PART) {
      float s = 0.f;
      for (int g = 0; g < G; g++) s += partials[g * IN_PART + t];
      s_sums[t] = s;
    }
    __syncthreads();
  };
  auto applyStep = [&]() __attribute__((always_inline)) {
    for (int i = t; i < n; i += 256) initApplyStepPoint(i, isGood, isGood_new, idepth, idepth_new, iR, energy, energy_new, lastHessian, lastHessian_new);
    cur ^= 1;
  };

  if (t == 0) {
    for (int k = 0; k < 7; k++) s_c.pose[k] = state->pose7[k];
    s_c.aff[0] = state->aff[0]; s_c.aff[1] = state->aff[1];
    s_c.snapped = state->snapped;
    s_c.lambda = 0.1; s_c.fails = 0; s_c.it = 0; s_c.quit = 0; s_c.accept = 0; s_c.cur_sys = 0; s_c.tests = 0;
    makeArgs(s_c.pose, s_c.aff);
  }
  // resetPoints (:891-918)
  for (int i = t; i < n; i += 256) initResetPoint(i, idepth, idepth_new, energy);
  if (V.is_top_level) {
    InitSweepResetTop body;
    body.idepth = idepth; body.idepth_new = idepth_new;
    initLmSweep<256>(n, V.sweep_levels, level_begin, order, neighbours, iR, isGood, s_iR, s_good, body);
  }
  __syncthreads();
  // the first evaluation and applyStep (:134-135)
  evaluate();
  if (t == 0) {
    InitLmSys& C = s_sys[0];
    initTail(poseFrom7(s_c.pose), n, V.alphaW, V.alphaK, V.priorY, V.priorX, s_sums, C.H, C.b, C.Hsc, C.bsc, C.res3, s_c.tlog);
  }
  applyStep();
  int swaps = 1;

  for (int round = 0; round <= V.max_iterations; round++) {   // (the quit rule leaves at iteration == max_iterations at the latest: this bound is the same one)
    if (t == 0) {
      const InitLmSys& C = s_sys[s_c.cur_sys];
      initLmControl(C.H, C.b, C.Hsc, C.bsc, s_c.lambda, V.wl * V.hl, V.wM8, V.fix_affine, s_c.pose, s_c.aff, s_ws, s_c.inc, &s_c.incNorm, s_c.pose_new, s_c.aff_new);
      makeArgs(s_c.pose_new, s_c.aff_new);
    }
    __syncthreads();
    const float lambda = s_c.lambda;
    const int snapped = s_c.snapped;
    {
      InitInc8 inc;
#pragma unroll
      for (int k = 0; k < 8; k++) inc.v[k] = s_c.inc[k];
      const float* Jb = cur ? jb1 : jb0;
      for (int i = t; i < n; i += 256) initDoStepPoint(i, lambda, inc, isGood, Jb, maxstep, idepth, idepth_new);
    }
    __syncthreads();
    evaluate();
    if (snapped) {   // calcEC (:650-670) in k_init_ec's and k_init_ec_final's shape
      for (int bx = 0; bx < G; bx++) {
        initEcPartialBody(n, isGood_new, idepth, idepth_new, iR, ecpartials, bx, G);
        __syncthreads();
      }
      if (t < 64) initEcFinalBody(G, ecpartials, s_ecsum);
      __syncthreads();
    }
    // the new system's two matrices for the trace, before lane 0 decides
    if (t == 0) {
      InitLmSys& C = s_sys[s_c.cur_sys];
      InitLmSys& N = s_sys[s_c.cur_sys ^ 1];
      initTail(poseFrom7(s_c.pose_new), n, V.alphaW, V.alphaK, V.priorY, V.priorX, s_sums, N.H, N.b, N.Hsc, N.bsc, N.res3, s_c.tlog);
      if (snapped) { s_c.ec3[0] = V.couplingWeight * s_ecsum[0]; s_c.ec3[1] = V.couplingWeight * s_ecsum[1]; s_c.ec3[2] = s_ecsum[2]; }
      else { s_c.ec3[0] = 0; s_c.ec3[1] = 0; s_c.ec3[2] = (float)n; }   // (:652)
      const float eNew = (N.res3[0] + N.res3[1] + s_c.ec3[1]);
      const float eOld = (C.res3[0] + C.res3[1] + s_c.ec3[0]);
      const bool accept = eOld > eNew;
      s_c.eOld = eOld; s_c.eNew = eNew; s_c.accept = accept; s_c.lambda_used = s_c.lambda;
      if (trace) {
        InitLmTraceRec& R = trace[V.trace_base + s_c.tests];
        R.d[0] = s_c.incNorm;
        for (int k = 0; k < 7; k++) { R.d[1 + k] = s_c.pose[k]; R.d[10 + k] = s_c.pose_new[k]; }
        R.d[8] = s_c.aff[0]; R.d[9] = s_c.aff[1]; R.d[17] = s_c.aff_new[0]; R.d[18] = s_c.aff_new[1]; R.d[19] = 0;
        R.f[0] = (float)V.lvl; R.f[1] = (float)s_c.it; R.f[2] = s_c.lambda; R.f[3] = accept ? 1.0f : 0.0f;
        for (int k = 0; k < 8; k++) R.f[5 + k] = s_c.inc[k];
        for (int k = 0; k < 3; k++) { R.f[13 + k] = C.res3[k]; R.f[16 + k] = N.res3[k]; R.f[19 + k] = s_c.ec3[k]; R.f[24 + k] = s_c.tlog[k]; }
        R.f[22] = eOld; R.f[23] = eNew;
        for (int k = 0; k < 8; k++) { R.f[96 + k] = N.b[k]; R.f[168 + k] = N.bsc[k]; }
      }
      if (accept) {
        if (N.res3[1] == V.alphaK * n) s_c.snapped = 1;
        s_c.cur_sys ^= 1;
        for (int k = 0; k < 7; k++) s_c.pose[k] = s_c.pose_new[k];
        s_c.aff[0] = s_c.aff_new[0]; s_c.aff[1] = s_c.aff_new[1];
      }
      s_c.quit = initLmRule(accept, s_c.incNorm, s_c.it, V.max_iterations, &s_c.lambda, &s_c.fails);
      if (trace) {
        InitLmTraceRec& R = trace[V.trace_base + s_c.tests];
        R.f[4] = (float)s_c.snapped; R.f[27] = (float)s_c.fails; R.f[28] = s_c.lambda; R.f[29] = (float)s_c.quit; R.f[30] = 0; R.f[31] = 0;
      }
    }
    __syncthreads();
    if (trace && t >= 64 && t < 192) {   // H and Hsc of the new evaluation as the tail left them (cur_sys names it after an accept, its twin after a reject)
      const InitLmSys& N = s_sys[s_c.accept ? s_c.cur_sys : (s_c.cur_sys ^ 1)];
      InitLmTraceRec& R = trace[V.trace_base + s_c.tests];
      const int k = t - 64;
      if (k < 64) R.f[32 + k] = N.H[k]; else R.f[104 + k - 64] = N.Hsc[k - 64];
    }
    const int accept = s_c.accept, quit = s_c.quit, now_snapped = s_c.snapped;
    __syncthreads();
    if (t == 0) { s_c.tests++; if (!quit) s_c.it++; }
    if (accept) {
      applyStep();
      swaps++;
      if (now_snapped) {   // optReg (:671-704)
        InitSweepOptReg body;
        body.regWeight = V.regWeight; body.idepth = idepth;
        initLmSweep<256>(n, V.sweep_levels, level_begin, order, neighbours, iR, isGood, s_iR, s_good, body);
      }
    }
    __syncthreads();
    if (quit) break;
  }

  // the two JbBuffers change places once per applyStep; after an odd number their contents do once more, so that the handle's JbBuffer is where it was
  if (swaps & 1)
    for (int k = t; k < 10 * n; k += 256) { const float a = jb0[k]; jb0[k] = jb1[k]; jb1[k] = a; }
  if (t == 0) {
    for (int k = 0; k < 7; k++) state->pose7[k] = s_c.pose[k];
    state->aff[0] = s_c.aff[0]; state->aff[1] = s_c.aff[1];
    state->snapped = s_c.snapped;
    InitLmOut& O = outs[V.out_index];
    const InitLmSys& C = s_sys[s_c.cur_sys];
    O.res3[0] = C.res3[0]; O.res3[1] = C.res3[1]; O.res3[2] = C.res3[2];
    O.iterations = s_c.it; O.tests = s_c.tests;
  }
}

inline __global__ void __launch_bounds__(256) k_init_lm(const InitLmProb* __restrict__ probs, InitLmState* __restrict__ state, InitLmOut* __restrict__ outs,
                                                 InitLmTraceRec* __restrict__ trace) {
  extern __shared__ float s_sweep[];
  __shared__ InitLmLds s_lm;
  initLmLevel(probs[blockIdx.x], state, outs, trace, s_sweep, s_lm);
}

// ------------------------------------------------------------------------------------------------ the frame around the levels (:100-114, propagateDown / Up's optReg)
// trackFrame's reset while the initializer has not snapped, for every level of the frame: workgroup (x, y) serves level y.  `snapped` is the record's, on the device.
inline __global__ void __launch_bounds__(256) k_init_lm_frame_begin(const InitLmProb* __restrict__ probs, InitLmState* __restrict__ state) {
  if (state->snapped) return;
  const InitLmProb& V = probs[blockIdx.y];
  float *iR = initGl(V.iR), *idepth_new = initGl(V.idepth_new), *lastHessian = initGl(V.lastHessian);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < V.n; i += gridDim.x * 256) initResetUnsnappedPoint(i, iR, idepth_new, lastHessian);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 3) state->pose7[threadIdx.x] = 0.0;   // thisToNext.translation().setZero() (:102); no workgroup reads the pose
}
// optReg of one level where the record says snapped: what propagateDown and propagateUp end in (:746, :776)
inline __global__ void __launch_bounds__(64) k_init_lm_opt_reg(const InitLmProb* __restrict__ probs, const InitLmState* __restrict__ state) {
  extern __shared__ float s_sweep[];
  if (!state->snapped) return;
  const InitLmProb& V = probs[blockIdx.x];
  InitSweepOptReg body;
  body.regWeight = V.regWeight; body.idepth = initGl(V.idepth);
  initLmSweep<64>(V.n, V.sweep_levels, initGl(V.level_begin), initGl(V.order), initGl(V.neighbours), initGl(V.iR), initGl(V.isGood), s_sweep,
                  reinterpret_cast<unsigned char*>(s_sweep + V.n), body);
}

// ------------------------------------------------------------------------------------------------ the control step alone (dmvio_hip_initializer_debug_lm_control)
struct InitLmControlIo {
  float H[64], b[8], Hsc[64], bsc[8], wM[8], lambda;
  int wh, fix_affine, pad;
  double pose7[7], aff[2];
  // out
  double incNorm, pose7_new[7], aff_new[2];
  float inc[8];
};
inline __global__ void __launch_bounds__(64) k_init_debug_lm_control(InitLmControlIo* __restrict__ io) {
  __shared__ InitLmWs s_ws;
  if (threadIdx.x != 0) return;
  initLmControl(io->H, io->b, io->Hsc, io->bsc, io->lambda, io->wh, io->wM, io->fix_affine, io->pose7, io->aff, s_ws, io->inc, &io->incNorm, io->pose7_new, io->aff_new);
}

}  // namespace dmv
