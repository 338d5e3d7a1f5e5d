// CoarseInitializer::trackFrame (src/dso/FullSystem/CoarseInitializer.cpp:100-114, 126-263, 708-747, 749-777) of W windows in ONE launch: workgroup w walks the whole frame
// of window w — the unsnapped reset, then from the top level down propagateDown, the conditional optReg and the level's LM loop, then propagateUp and the conditional optReg
// for the level pairs — with no host in between.  Every piece is the single call's own device body (initLmLevel: k_init_lm's; the per-point bodies of
// init_resident_kernels.hpp; initLmSweep), the per-point passes taken by a 256-thread stride: their operations are independent per point, so the stride gives the bits of the
// multi-workgroup launches of dmvio_hip_initializer_resident_track_frame.  Between two phases stands a workgroup barrier; all traffic of a window stays inside its workgroup.
#pragma once
#include "init_lm_kernels.hpp"

namespace dmv {

// One window.  Its levels are the InitLmProb records prob_base .. prob_base + n_levels - 1 in execution order (the top level first): parent[p] is level p's table into level
// p - 1 (unused for p = 0), child_begin[p] / children[p] / n_listed[p] level p's children lists as propagateUp into level p - 1 reads them.  Addressed with blockIdx.x;
// the pointers are read through initGl().
struct InitLmWin {
  const int *parent[DMV_MAX_LEVELS], *child_begin[DMV_MAX_LEVELS], *children[DMV_MAX_LEVELS];
  int n_listed[DMV_MAX_LEVELS];
  int n_levels, prob_base, state_slot, traced;   // traced: the window's levels write trace records (at their records' trace_base)
};

// optReg of one level by the whole workgroup: what propagateDown and propagateUp end in where the record says snapped (:746, :776)
__device__ __forceinline__ void initLmFrameOptReg(const InitLmProb& V, float* __restrict__ s_sweep) {
  InitSweepOptReg body;
  body.regWeight = V.regWeight; body.idepth = initGl(V.idepth);
  initLmSweep<256>(V.n, V.sweep_levels, initGl(V.level_begin), initGl(V.order), initGl(V.neighbours), initGl(V.iR), initGl(V.isGood), s_sweep,
                   reinterpret_cast<unsigned char*>(s_sweep + V.n), body);
}

// grid W, 256 threads, dynamic LDS for the largest level of the call.  records: the batch's LM records, one per state slot; state_in (NULL: no window brings a state): per
// window the incoming state, taken where its `pad` is set; state_out: per window the record as the frame left it.
inline __global__ void __launch_bounds__(256) k_init_lm_frame_b(const InitLmWin* __restrict__ wins, const InitLmProb* __restrict__ probs, InitLmState* __restrict__ records,
                                                         const InitLmState* __restrict__ state_in, InitLmState* __restrict__ state_out, InitLmOut* __restrict__ outs,
                                                         InitLmTraceRec* __restrict__ trace_all) {
  extern __shared__ float s_sweep[];
  __shared__ InitLmLds s_lm;
  const InitLmWin& Wn = wins[blockIdx.x];
  const int t = threadIdx.x, P = Wn.n_levels;
  const InitLmProb* __restrict__ lv = probs + Wn.prob_base;
  InitLmState* __restrict__ state = records + Wn.state_slot;
  InitLmTraceRec* __restrict__ trace = Wn.traced ? trace_all : nullptr;

  if (state_in && state_in[blockIdx.x].pad) {
    if (t == 0) { InitLmState S = state_in[blockIdx.x]; S.pad = 0; *state = S; }
    __syncthreads();
  }
  // trackFrame's reset while the initializer has not snapped (:100-114)
  if (!state->snapped) {
    for (int p = 0; p < P; p++) {
      const InitLmProb& V = lv[p];
      float *iR = initGl(V.iR), *idepth_new = initGl(V.idepth_new), *lastHessian = initGl(V.lastHessian);
      for (int i = t; i < V.n; i += 256) initResetUnsnappedPoint(i, iR, idepth_new, lastHessian);
    }
    if (t < 3) state->pose7[t] = 0.0;   // thisToNext.translation().setZero() (:102)
  }
  __syncthreads();

  for (int p = 0; p < P; p++) {
    const InitLmProb& V = lv[p];
    if (p > 0 && V.n > 0) {   // propagateDown from the level above (:749-777)
      const InitLmProb& U = lv[p - 1];
      const int* parent = initGl(Wn.parent[p]);
      const unsigned char* par_good = initGl(U.isGood);
      const float *par_iR = initGl(U.iR), *par_lh = initGl(U.lastHessian);
      unsigned char* isGood = initGl(V.isGood);
      float *iR = initGl(V.iR), *idepth = initGl(V.idepth), *idepth_new = initGl(V.idepth_new), *lastHessian = initGl(V.lastHessian);
      for (int i = t; i < V.n; i += 256) initPropagateDownPoint(i, parent, par_good, par_iR, par_lh, isGood, iR, idepth, idepth_new, lastHessian);
      if (state->snapped) initLmFrameOptReg(V, s_sweep);
      __syncthreads();
    }
    initLmLevel(V, state, outs, trace, s_sweep, s_lm);
    __syncthreads();
  }

  for (int p = P - 1; p > 0; p--) {   // propagateUp from level lv[p] into lv[p - 1], the lowest pair first (:262-263, :708-747)
    const InitLmProb &Lo = lv[p], &V = lv[p - 1];
    if (V.n == 0) continue;
    const int *child_begin = initGl(Wn.child_begin[p]), *children = initGl(Wn.children[p]);
    const unsigned char* src_good = initGl(Lo.isGood);
    const float *src_iR = initGl(Lo.iR), *src_lh = initGl(Lo.lastHessian);
    float *iR = initGl(V.iR), *idepth = initGl(V.idepth);
    unsigned char* isGood = initGl(V.isGood);
    const int n_listed = Wn.n_listed[p];
    for (int i = t; i < V.n; i += 256) initPropagateUpPoint(i, n_listed, child_begin, children, src_good, src_iR, src_lh, iR, idepth, isGood);
    if (state->snapped) initLmFrameOptReg(V, s_sweep);
    __syncthreads();
  }
  if (t == 0) state_out[blockIdx.x] = *state;
}

}  // namespace dmv
