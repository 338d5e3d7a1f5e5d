// The uniform head and the tail of CoarseInitializer::calcResAndGS (CoarseInitializer.cpp:331-624) around the evaluation kernel: what is made from the pose before the launch
// (initMakeArgsAt) and what is made from the IN_PART sums behind it (initTail).  __host__ __device__: the host-driven calls (capi_init.hip, capi_init_resident.hip) run them
// on the host, the device-resident LM loop (init_lm_kernels.hpp) on lane 0 of its workgroup.  Plain single- and double-precision arithmetic in the order written, so both sides
// give the same bits, with two exceptions that reach libm: exp(aff.a), and the pose's logarithm (atan, tan), whose device versions may differ from glibc's in the last place.
#pragma once
#include "lie_dev.h"
#include "init_types.hpp"

namespace dmv {

// alpha energy (CoarseInitializer.cpp:497-535); EAlpha.A is identically 0 in the reference.  Returns alphaOpt.
DMV_HD float initAlpha(const Pose& T, int n, float alphaW, float alphaK, float* alphaEnergy_out) {
  const double tsq = T.t[0] * T.t[0] + T.t[1] * T.t[1] + T.t[2] * T.t[2];
  float alphaEnergy = alphaW * (0.0f + tsq * n);
  float alphaOpt;
  if (alphaEnergy > alphaK * n) { alphaOpt = 0; alphaEnergy = alphaK * n; }
  else alphaOpt = alphaW;
  *alphaEnergy_out = alphaEnergy;
  return alphaOpt;
}
// the uniform inputs of the evaluation kernel for a level of wl x hl pixels
DMV_HD InitArgs initMakeArgsAt(int wl, int hl, const double Ki9[9], const float fxfycxcy_lvl[4], const Pose& T, const double aff_ab[2], int n, float alphaW, float alphaK,
                               float couplingWeight) {
  InitArgs A;
  double Rd[9];
  quatToR(T.q, Rd);
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 3; q++) A.RKi[r * 3 + q] = (float)(Rd[r * 3 + 0] * Ki9[q] + Rd[r * 3 + 1] * Ki9[3 + q] + Rd[r * 3 + 2] * Ki9[6 + q]);
  for (int i = 0; i < 3; i++) A.t[i] = (float)T.t[i];
  A.aff0 = (float)dexp(aff_ab[0]); A.aff1 = (float)aff_ab[1];
  A.fxl = fxfycxcy_lvl[0]; A.fyl = fxfycxcy_lvl[1]; A.cxl = fxfycxcy_lvl[2]; A.cyl = fxfycxcy_lvl[3];
  A.wl = wl; A.hl = hl;
  A.couplingWeight = couplingWeight; A.huberTH = 9.0f;
  float alphaEnergy;
  A.alphaOpt = initAlpha(T, n, alphaW, alphaK, &alphaEnergy);
  return A;
}
// where sums[0 .. 44] (and [45 .. 89]) keep entry (r, q) of the symmetric 9x9: the upper triangle row by row
DMV_HD int initTri9(int r, int q) {
  const int a = r < q ? r : q, b = r < q ? q : r;
  return a * 9 - (a * (a - 1)) / 2 + (b - a);
}
// the tail of calcResAndGS: the alpha energy and alphaOpt (:497-535), the two upper triangles unpacked, then :582-613.  tlog3 (may be NULL): the float translation part of
// the pose's logarithm that went into b[0..2].
DMV_HD void initTail(const Pose& T, int n, float alphaW, float alphaK, double priorY, double priorX, const float* sums /* IN_PART */, float* H_out64, float* b_out8, float* H_sc64,
                     float* b_sc8, float res3[3], float* tlog3) {
  float alphaEnergy;
  const float alphaOpt = initAlpha(T, n, alphaW, alphaK, &alphaEnergy);
  for (int r = 0; r < 8; r++) {
    for (int q = 0; q < 8; q++) { const int k = initTri9(r, q); H_out64[r * 8 + q] = sums[k]; H_sc64[r * 8 + q] = sums[45 + k]; }
    const int k8 = initTri9(r, 8);
    b_out8[r] = sums[k8]; b_sc8[r] = sums[45 + k8];
  }
  H_out64[0] += alphaOpt * n; H_out64[9] += alphaOpt * n; H_out64[18] += alphaOpt * n;
  double lg[6];
  poseLog(T, lg);
  const float tlog[3] = {(float)lg[0], (float)lg[1], (float)lg[2]};
  b_out8[0] += tlog[0] * alphaOpt * n; b_out8[1] += tlog[1] * alphaOpt * n; b_out8[2] += tlog[2] * alphaOpt * n;
  H_out64[9] += priorY; b_out8[1] += priorY * T.t[1];
  H_out64[0] += priorX; b_out8[0] += priorX * T.t[0];
  res3[0] = sums[90]; res3[1] = alphaEnergy; res3[2] = (float)(2 * (size_t)n);   // accE[0].num: every point once per loop (:351-470, :503-516)
  if (tlog3) { tlog3[0] = tlog[0]; tlog3[1] = tlog[1]; tlog3[2] = tlog[2]; }
}

}  // namespace dmv
