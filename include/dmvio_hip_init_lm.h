/* The initializer's Levenberg-Marquardt loop on the device: an extension of the C ABI of libdmvio_hip.so (dmvio_hip.h) on top of the resident initializer
 * (dmvio_hip_init_resident.h), in a header of its own.  Include it beside those two; the entry points live in the same library and take the same handles. */
#ifndef DMVIO_HIP_INIT_LM_H
#define DMVIO_HIP_INIT_LM_H
#include "dmvio_hip.h"
#include "dmvio_hip_init_resident.h"
#ifdef __cplusplus
extern "C" {
#endif

/* CoarseInitializer::trackFrame (CoarseInitializer.cpp:85-281) on handles that hold a resident point set: the loop that strings the resident passes together — the 6x6 / 8x8
 * solve, SE3::exp, the accept test, the lambda / fails / quit rules — runs on the device, ONE workgroup per level, ONE launch per level whatever the iteration count.
 *
 * The LM state {refToNew (7 doubles: t, then the quaternion x y z w), refToNew_aff (a, b), snapped} lives in a device record of the context.  The calls pass it as ten
 * doubles, state10 = pose7 | a | b | snapped (0 or 1).  state_in10 == NULL: continue from what the previous call left in the record (refused while the record holds
 * nothing).  state_out10 == NULL: enqueue only, no download and no wait; the other outputs are then not written.
 *
 *   lm_control_host   :159-185, pure host, no context.  Hl = H with its diagonal times (1 + lambda), minus Hsc / (1 + lambda); bl likewise; both scaled by wM8 (the diagonal
 *                     of wM) and 0.01f / wh (wh = w[lvl] * h[lvl]); inc8 = -wM * Hl^-1 * bl by a float LDLT with diagonal pivoting — the 6x6 head with a zero tail when
 *                     fix_affine != 0, the full 8x8 otherwise; incNorm = |inc8| (float sum, float sqrt); refToNew7_new = SE3::exp(inc8[0..5]) * refToNew7;
 *                     aff_ab_new = aff_ab + inc8[6..7].  Float operations in the order the compiled reference takes them: a trackFrame driven by this function on the host
 *                     reproduces the reference's own trackFrame bit for bit, pose, affine pair and every point (tests/golden/init_lm_frames.npz, both branches); inc8
 *                     and incNorm have no recorded reference numbers of their own.  H64 / Hsc64: row-major 8x8, of which the lower triangle is read by the solve.
 *   debug_lm_control  the same function on the device: one wavefront, lane 0, on the context's stream; one upload, one download, one wait.  For tests: inc8 and incNorm equal
 *                     the host's bit for bit, the pose to the rounding of the device's sin / cos.
 *   resident_track_level   :133-253 for one level: resetPoints (with the top-level sweep when is_top_level != 0), the first evaluation, applyStep, then the whole while(true)
 *                     loop.  On accept: snapped becomes 1 where resNew[1] == alphaK * n, applyStep, optReg when snapped, lambda * 0.5; else fails + 1, lambda * 4; the loop
 *                     quits when !(incNorm > 1e-4), iteration >= max_iterations or fails >= 2.  res3 (may be NULL): resOld when the loop quit; iterations (may be NULL): the
 *                     iteration it quit in.  ONE launch, at most one upload (the problem record and the state, where either changed), at most ONE download and ONE wait.
 *   resident_track_frame   :100-114 and :126-263 over the n_levels handles of one context, levels[k] being level k: the unsnapped reset of every level with refToNew's
 *                     translation zeroed where the incoming state is not snapped; from the top level down propagateDown (:749-777) then the level's loop; propagateUp
 *                     (:708-747) for the levels 0 .. n_levels - 2.  Level l starts from the pose level l + 1 left, with no host in between; whether optReg runs behind a
 *                     propagate call is read from the record's snapped on the device.  Ki9_levels: 9 doubles, fxfycxcy_levels: 4 floats, max_iterations: one int, res3_levels:
 *                     3 floats, iterations_levels: one int per level (the last two may be NULL).  Launches: 1 (the reset) + n_levels (the loops) + for each of the
 *                     n_levels - 1 level pairs a propagateDown, a propagateUp and behind each the conditional optReg: 5 n_levels - 3 where no level is empty.  ONE download,
 *                     ONE wait.  Returns snapped (0 / 1) of the outgoing state, 0 when state_out10 == NULL, < 0 on failure.  The exposure-based start of aff (:121-122),
 *                     frameID / snappedAt and trackFrame's return value stay the caller's.
 *   lm_last_work      launches, uploads, downloads and waits of the last track_level / track_frame of the context (any pointer may be NULL).  A refused call counts nothing
 *                     and leaves the figures as they were.
 *
 * The trace (trace_d == NULL: none): one record per accept test in the order the tests are made, trace_capacity records of room in each array, *trace_records = how many were
 * written.  Per record INIT_LM_TRACE_D doubles — [0] incNorm, [1..7] the entering pose, [8..9] the entering aff, [10..16] the new pose, [17..18] the new aff — and
 * INIT_LM_TRACE_F floats — [0] lvl, [1] iteration, [2] lambda of the step, [3] accept, [4] snapped after the test, [5..12] inc8, [13..15] resOld, [16..18] resNew, [19..21]
 * calcEC's three values, [22] eTotalOld, [23] eTotalNew, [24..26] the float translation part of log(new pose) that went into b[0..2], [27] fails after the test, [28] lambda
 * after it, [29] quit, [32..95] H, [96..103] b, [104..167] Hsc, [168..175] bsc of the new evaluation as calcResAndGS's tail left them.
 *
 * What the device loop may differ in from the host-driven one: the pose algebra (the device's sin / cos are not glibc's), exp(a), and the logarithm that feeds b[0..2] — an
 * ulp each.  Everything per point, the 91 sums of an evaluation and calcEC's three sums have the bits of dmvio_hip_initializer_resident_calc AT THE POSE THE DEVICE USED
 * (the same device bodies in the same order), and inc8 / incNorm those of lm_control_host on the traced H, b, Hsc, bsc.  Afterwards the handle is in the state the
 * host-driven calls would have left, the JbBuffers included.
 *
 * Each call is refused as a whole, before anything is enqueued and with handles, record and outputs untouched: a NULL handle or array (but those said to be optional); a handle
 * without resident state; lvl, a slot or max_iterations out of range (max_iterations in [0, 64]: the trace has a bound); n_levels outside [1, the context's levels]; handles
 * of different contexts or one handle named twice; a lower level without a parent table, or with a parent at or above the upper level's n; any point — good or not: the top
 * level's resetPoints and a frame's propagateDown revive points inside the call — outside [2, w_lvl - 3) x [2, h_lvl - 3) by the host copy of (u, v), in track_frame and in a
 * track_level with is_top_level; in a track_level of a lower level, which revives nothing, the range condition of resident_calc: where the host copy shows a point outside,
 * the GOOD points outside are counted on the device first, in a download and a wait of their own, and a non-zero count refuses the call before the loop is enqueued; a level whose loop needs more LDS than the device allows a workgroup (the sweeps'
 * 5 n bytes beside the loop's own; the message names n and the limit); state_in10 == NULL while the record is empty; a trace without room for every test the call can make
 * (the sum of max_iterations + 1 over its levels). */
#define DMVIO_HIP_INIT_LM_TRACE_D 20
#define DMVIO_HIP_INIT_LM_TRACE_F 176
int dmvio_hip_initializer_lm_control_host(const float* H64, const float* b8, const float* Hsc64, const float* bsc8, float lambda, int wh, const float* wM8, int fix_affine,
                                          const double* refToNew7, const double* aff_ab, float* inc8, double* incNorm, double* refToNew7_new, double* aff_ab_new);
int dmvio_hip_initializer_debug_lm_control(dmvio_hip_ctx* ctx, const float* H64, const float* b8, const float* Hsc64, const float* bsc8, float lambda, int wh, const float* wM8,
                                           int fix_affine, const double* refToNew7, const double* aff_ab, float* inc8, double* incNorm, double* refToNew7_new,
                                           double* aff_ab_new);
int dmvio_hip_initializer_resident_track_level(dmvio_hip_initializer* ini, int lvl, int first_slot, int new_slot, const double* Ki9, const float* fxfycxcy_lvl, float alphaW,
                                               float alphaK, float regWeight, float couplingWeight, double priorY, double priorX, const float* wM8, int fix_affine,
                                               int max_iterations, int is_top_level, const double* state_in10, double* state_out10, float* res3, int* iterations,
                                               int trace_capacity, double* trace_d, float* trace_f, int* trace_records);
int dmvio_hip_initializer_resident_track_frame(dmvio_hip_initializer* const* levels, int n_levels, int first_slot, int new_slot, const double* Ki9_levels,
                                               const float* fxfycxcy_levels, float alphaW, float alphaK, float regWeight, float couplingWeight, double priorY, double priorX,
                                               const float* wM8, int fix_affine, const int* max_iterations, const double* state_in10, double* state_out10, float* res3_levels,
                                               int* iterations_levels, int trace_capacity, double* trace_d, float* trace_f, int* trace_records);
int dmvio_hip_initializer_lm_last_work(dmvio_hip_ctx* ctx, int* launches, int* uploads, int* downloads, int* waits);

#ifdef __cplusplus
}
#endif
#endif
