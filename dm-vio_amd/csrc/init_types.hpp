// What the initializer's units share without the kernels: the layout of a partial and the argument records of the evaluation (init_kernels.hpp), which the resident
// unit (capi_init_resident.hip) fills for a launch the evaluation's own unit (capi_init.hip) makes.
#pragma once

namespace dmv {

enum { IN_STRIDE = 66, IN_ROWS = 16, IN_WAVE_FLOATS = IN_ROWS * IN_STRIDE + 64, IN_PART = 96 };   // partial: 45 H + 45 SC + E + pad

struct InitPts {   // struct Pnt (CoarseInitializer.h:44-83), structure of arrays
  int n;
  const float *u, *v, *idepth_new, *iR, *energy /* 2n */, *outlierTH;
  const unsigned char* isGood;
  float *energy_new /* 2n */, *maxstep, *lastHessian_new, *JbBuffer_new /* 10n */;
  unsigned char* isGood_new;
};
struct InitArgs {
  float RKi[9], t[3], aff0, aff1;   // (R * Ki).cast<float>(), translation, (exp(a), b)
  float fxl, fyl, cxl, cyl;
  int wl, hl;
  float alphaOpt, couplingWeight, huberTH;
};

}  // namespace dmv
