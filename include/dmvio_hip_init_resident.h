/* The resident initializer: an extension of the C ABI of libdmvio_hip.so (dmvio_hip.h), in a header of its own.  Include it beside dmvio_hip.h; the entry points
 * live in the same library and take the same handles. */
#ifndef DMVIO_HIP_INIT_RESIDENT_H
#define DMVIO_HIP_INIT_RESIDENT_H
#include "dmvio_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The point set of a level resident on the device, and the per-point passes of CoarseInitializer::trackFrame on it (CoarseInitializer.cpp:85-281).  After set_resident
 * all of struct Pnt that the passes touch and both JbBuffers live in device memory; the calls below run the reference's loops there, and nothing per point crosses PCIe
 * until get_state.  The LM loop itself, the 8x8 solve and the pose update stay the caller's, on the host (the loop can also run on the device, on the same resident
 * state: dmvio_hip_init_lm.h).  setFirst and makeNN, which create the point sets, can run on the device too and hand them over without an upload: dmvio_hip_init_first.h
 * (dmvio_hip_initializer_set_first leaves the state set_resident would).  Every per-point value has the reference's bits.
 *   set_resident        one packed upload of the point set (Pnt's u, v, idepth, iR, isGood, energy, outlierTH, lastHessian, neighbours[10], parent; parent NULL on the top
 *                       level), idepth_new = idepth, the *_new fields, maxstep and both JbBuffers zeroed.  Builds, on the host, the static schedule of the ordered sweeps
 *                       and the children lists of propagateUp.  The handle's non-resident state (set_points, calc_res_and_gs, the batched calls) is not touched, nor does any of
 *                       those calls touch the resident state.
 *   resident_reset_unsnapped   :100-114  (iR = idepth_new = 1, lastHessian = 0)
 *   resident_reset_points      :891-918  (energy = 0, idepth_new = idepth; is_top_level != 0: the sweep that revives bad points from their good neighbours, in index order)
 *   resident_do_step           :919-947  (reads the current JbBuffer; inc8: the Vec8f)
 *   resident_apply_step        :948-965  (the JbBuffer swap is a pointer swap)
 *   resident_opt_reg           :671-704  (the caller passes it only when snapped, as :675; the in-place median sweep in index order)
 *   resident_propagate_down    :749-777  (src: the upper level, dst: the lower one, whose parent table is used; includes optReg of dst when snapped != 0)
 *   resident_propagate_up      :708-747  (src: the lower level, whose parent table is used, dst: the upper one; includes optReg of dst when snapped != 0)
 *   resident_calc              :331-624 on the resident points, then calcEC :650-670.  H_out64 .. res3 have the bits of dmvio_hip_initializer_calc_res_and_gs on the same
 *                       inputs (the same kernels on the same grid); idepth_new is read from, and the five per-point results are written to, the resident arrays (the
 *                       JbBuffer that is not current).  ec3 (may be NULL) = (couplingWeight * sum rOld^2, couplingWeight * sum rNew^2, count) over the accepted points,
 *                       summed in a fixed shape on the device (each term passes through at most ceil(n / (G * 256)) + 17 additions, G = max(1, min(256, (n + 255) / 256)));
 *                       (0, 0, n) without a launch when snapped == 0, as :652.  ONE download of 100 floats, one wait.
 *   resident_get_state  every field of Pnt a pass writes, maxstep and the current JbBuffer; each pointer may be NULL.  One download, one wait.
 *   resident_set_state  the mirror of get_state, plus the JbBuffer that is not current: the fields given (each pointer may be NULL) replace the resident ones, one upload per
 *                       field given, no wait.  For tests, and for a caller that runs a pass on the host between get_state and set_state (set_resident would zero the
 *                       JbBuffers the next doStep reads).
 *   resident_last_work  launches, uploads, downloads and waits counted since the last resident_calc or resident_get_state returned (those calls' own included): an LM
 *                       iteration of do_step + calc reports 0 uploads, 1 download, 1 wait.  A refused call counts nothing.
 * All but calc and get_state only enqueue.  All run under the context's lock on the context's stream.
 * The two sweeps run as ONE workgroup of one wavefront with iR and isGood of the level in LDS (5 n bytes): set_resident refuses a point set for which that exceeds what the
 * device offers a workgroup, with a message naming n and the limit.
 * Range check of calc: as the single call's, but isGood lives on the device.  Where the host copy of (u, v) shows no point outside [2, w_lvl - 3) x [2, h_lvl - 3) — every
 * set setFirst makes — nothing is needed.  Otherwise the good points outside are counted on the device first, in a download and a wait of their own, and a non-zero count
 * refuses the call before the evaluation is launched, outputs untouched: the one difference from the single call's "before anything is launched".
 * Each call is refused as a whole, before anything is enqueued and with handles and outputs untouched: a NULL handle or a NULL array (but those said to be optional); n < 0 or
 * above the handle's capacity; a neighbour that is neither -1 nor in [0, n); a parent below 0 or at or above w * h; the LDS limit; a resident_ call on a handle without
 * resident state; lvl or a slot out of range; in a propagate call, handles of different contexts, a lower level without parent table, or a parent at or above the upper
 * level's n. */
int dmvio_hip_initializer_set_resident(dmvio_hip_initializer* ini, int n, const float* u, const float* v, const float* idepth, const float* iR, const unsigned char* isGood,
                                       const float* energy2, const float* outlierTH, const float* lastHessian, const int* neighbours10, const int* parent);
int dmvio_hip_initializer_resident_reset_unsnapped(dmvio_hip_initializer* ini);
int dmvio_hip_initializer_resident_reset_points(dmvio_hip_initializer* ini, int is_top_level);
int dmvio_hip_initializer_resident_do_step(dmvio_hip_initializer* ini, float lambda, const float inc8[8]);
int dmvio_hip_initializer_resident_apply_step(dmvio_hip_initializer* ini);
int dmvio_hip_initializer_resident_opt_reg(dmvio_hip_initializer* ini, float regWeight);
int dmvio_hip_initializer_resident_propagate_down(dmvio_hip_initializer* src, dmvio_hip_initializer* dst, float regWeight, int snapped);
int dmvio_hip_initializer_resident_propagate_up(dmvio_hip_initializer* src, dmvio_hip_initializer* dst, float regWeight, int snapped);
int dmvio_hip_initializer_resident_calc(dmvio_hip_initializer* ini, int lvl, int first_slot, int new_slot, const double Ki9[9], const float fxfycxcy_lvl[4],
                                        const double refToNew7[7], const double aff_ab[2], float alphaW, float alphaK, float couplingWeight, double priorY, double priorX,
                                        int snapped, float* H_out64, float* b_out8, float* H_sc64, float* b_sc8, float res3[3], float* ec3);
int dmvio_hip_initializer_resident_get_state(dmvio_hip_initializer* ini, float* idepth, float* iR, unsigned char* isGood, float* energy2, float* lastHessian,
                                             float* idepth_new, unsigned char* isGood_new, float* energy_new2, float* lastHessian_new, float* maxstep, float* JbBuffer10);
int dmvio_hip_initializer_resident_set_state(dmvio_hip_initializer* ini, const float* idepth, const float* iR, const unsigned char* isGood, const float* energy2,
                                             const float* lastHessian, const float* idepth_new, const unsigned char* isGood_new, const float* energy_new2,
                                             const float* lastHessian_new, const float* maxstep, const float* JbBuffer10, const float* JbBuffer_new10);
int dmvio_hip_initializer_resident_last_work(dmvio_hip_initializer* ini, int* launches, int* uploads, int* downloads, int* waits);

#ifdef __cplusplus
}
#endif
#endif
