// the immature points' structure-of-arrays and settings: shared by the kernels of immature_kernels.hpp and activate_kernels.hpp
#pragma once

namespace dmv {

enum { IPS_GOOD = 0, IPS_OOB, IPS_OUTLIER, IPS_SKIPPED, IPS_BADCONDITION, IPS_UNINITIALIZED };

struct ImmaturePts {
  int n;
  // static part (constructor)
  float *u, *v;              // pixel position in the host (integers stored as float, ImmaturePoint.h:66)
  int* host;                 // index into the per-host tables of a trace call
  float *color, *weights;    // n x 8
  float* gradH;              // n x 4 (00 01 10 11)
  float* energyTH;
  // mutable part
  float *idepth_min, *idepth_max, *quality, *lastTraceUV /* n x 2 */, *lastTracePixelInterval;
  int* lastTraceStatus;
  float* my_type;            // ImmaturePoint::my_type (ImmaturePoint.h:73): the selector's map value, 1 for points added without one
};

struct ImmatureSettings {
  float outlierTH = 12 * 12, outlierTHSumComponent = 50 * 50, overallEnergyTHWeight = 1;
  float maxPixSearch = 0.027f, huberTH = 9;
  int minTraceTestRadius = 2, GNIterations = 3;
  float stepsize = 1.0f, GNThreshold = 0.1f, extraSlackOnTH = 1.2f, slackInterval = 1.5f, minImprovementFactor = 2;
};

}  // namespace dmv
