// struct dmvio_hip_initializer, shared by the initializer's units: capi_init.hip (calcResAndGS, one window and W windows per call) defines the handle's entry points and the
// evaluation's launch; capi_init_resident.hip hangs the resident point set on the handle (init_resident_state.h) and borrows the launch and the host tail declared below;
// capi_init_lm.hip and capi_init_lm_batch.hip run trackFrame's LM loop on that point set, capi_init_first.hip makes it on the device (dmvInitResidentAdopt).  Also what
// all of them share of the device's limits: the evaluation's grid and the LDS allowance of a kernel.
#pragma once
#include <algorithm>
#include <vector>
#include "internal.h"
#include "lie_dev.h"
#include "init_types.hpp"

struct dmvio_hip_initializer_batch;
struct DmvInitResident;   // capi_init_resident.hip

struct dmvio_hip_initializer {
  dmvio_hip_ctx* ctx = nullptr;
  int capacity = 0, n = 0;
  // ONE device slab for the inputs and one for the per-point results, laid out per call for the n points of the level ([u | v | iR | outlierTH | energy(2) | idepth_new | isGood]
  // and [energy_new(2) | maxstep | lastHessian_new | JbBuffer_new(10) | isGood_new]); each crosses PCIe as ONE copy from / into pinned staging memory — a calcResAndGS call of
  // the initializer's LM loop is ~15 us of kernels, thirteen separate pageable copies cost ten times that
  float *d_in = nullptr, *d_res = nullptr, *h_in = nullptr, *h_res = nullptr;
  float *d_partials = nullptr, *d_out = nullptr, *h_out = nullptr;
  bool upload_pending = false;
  // where the point set of the last set_points lives on the device: d_in, or, after dmvio_hip_initializer_set_points_batch, this handle's part of that batch's slab (the
  // layout of d_in; `owner` is that batch).  Both are only touched under the context's lock.
  float* pts = nullptr;
  dmvio_hip_initializer_batch* owner = nullptr;
  std::vector<void*> allocs;
  // the point set of dmvio_hip_initializer_set_resident, apart from everything above: no existing call reads or writes it.  Only touched under the context's lock.
  DmvInitResident* resident = nullptr;
};
static inline size_t padn(int n) { return dmvPad(sizeof(float) * (size_t)n) / sizeof(float); }   // floats: every array of a slab starts on a 256-byte boundary
enum { IN_FLOATS = 7, RES_FLOATS = 14 };   // per point, + one byte each (isGood / isGood_new) at the end of the slab

// ---- capi_init.hip, for the resident unit
// the uniform inputs of the evaluation kernel
dmv::InitArgs initMakeArgs(const dmvio_hip_ctx* c, int lvl, const double Ki9[9], const float fxfycxcy_lvl[4], const dmv::Pose& T, const double aff_ab[2], int n, float alphaW,
                           float alphaK, float couplingWeight);
// the evaluation's grid for n points: of the single call, of every window of a batched one and of the resident calls, so the sums have the same bits wherever the points lie
enum { INIT_MAX_BLOCKS = 256 };
static inline int initGrid(int n) { return std::max(1, std::min((int)INIT_MAX_BLOCKS, (n + 255) / 256)); }
// k_init_partial on initGrid(P.n) workgroups and k_init_final behind it, on the context's stream; d_partials: INIT_MAX_BLOCKS x IN_PART floats, d_out: IN_PART
int initLaunchEval(dmvio_hip_ctx* c, int lvl, int first_slot, int new_slot, const dmv::InitPts& P, const dmv::InitArgs& A, float* d_partials, float* d_out);
// the host tail of calcResAndGS from the IN_PART downloaded sums
void initHostTail(const dmv::Pose& T, int n, float alphaW, float alphaK, double priorY, double priorX, const float* sums, float* H_out64, float* b_out8, float* H_sc64, float* b_sc8,
                  float res3[3]);
// ---- capi_init_resident.hip, for dmvio_hip_initializer_destroy (the stream has been waited for)
void dmvInitResidentRelease(dmvio_hip_initializer* m);
// ---- capi_init_resident.hip, for dmvio_hip_initializer_set_first (capi_init_first.hip); both under the context's lock.  dmvInitResidentCheck: what the install of a
// resident point set refuses of n points (the handle's capacity, the LDS of the ordered sweeps), the handle untouched.  dmvInitResidentAdopt: the resident state of
// setFirst's point set from lists on the device and their host copy.
int dmvInitResidentCheck(dmvio_hip_initializer* m, int n, const char* who);
int dmvInitResidentAdopt(dmvio_hip_initializer* m, int n, const float* d_u, const float* d_v, const int* d_nb, const int* d_parent, const float* h_u, const float* h_v,
                         const int* h_nb, const int* h_parent, float outlierTH, DmvWork* work);

// ---- the LDS a workgroup may have.  *limit: the device's figure (<= 0: it reports none).  With a kernel: *lds_static is what the kernel declares itself, and where the
// limit exceeds that, the kernel's dynamic allowance is raised to the rest.  The callers word their own refusals.
static inline hipError_t initLdsAllow(int device, int* limit, const void* kernel = nullptr, size_t* lds_static = nullptr) {
  *limit = 0;
  if (hipError_t e = hipDeviceGetAttribute(limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device)) return e;
  if (!kernel) return hipSuccess;
  hipFuncAttributes fa;
  if (hipError_t e = hipFuncGetAttributes(&fa, kernel)) return e;
  *lds_static = fa.sharedSizeBytes;
  if (*limit <= 0 || fa.sharedSizeBytes >= (size_t)*limit) return hipSuccess;
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, *limit - (int)fa.sharedSizeBytes);
}
