/* The initializer's Levenberg-Marquardt loop on the device, the frames of W windows per call: an extension of the C ABI of libdmvio_hip.so (dmvio_hip.h) beside
 * dmvio_hip_init_lm.h, in a header of its own.  The entry points live in the same library and take the same handles. */
#ifndef DMVIO_HIP_INIT_LM_BATCH_H
#define DMVIO_HIP_INIT_LM_BATCH_H
#include "dmvio_hip.h"
#include "dmvio_hip_init_resident.h"
#include "dmvio_hip_init_lm.h"
#ifdef __cplusplus
extern "C" {
#endif

/* CoarseInitializer::trackFrame (CoarseInitializer.cpp:100-114, 126-263, 708-747, 749-777) of W windows in ONE launch: one 256-thread workgroup per window walks that
 * window's whole frame — the unsnapped reset, from the top level down propagateDown, the conditional optReg and the level's LM loop, then propagateUp and the conditional
 * optReg for the level pairs — with no host in between.
 *
 * Every window ends exactly as its own dmvio_hip_initializer_resident_track_frame call on those handles, with that state and those arguments, would have left it:
 * state_out10, res3, iterations, every trace record, and every resident array of every level handle, the JbBuffers included.  The equality is bit for bit, the pose too: it is
 * the same device code with the same sin / cos, so none of the ulp allowances of the single call against a host-driven loop stand between the batched and the single call.
 * Single and batched calls mix freely on the same handles; the LM state crosses between them as the ten doubles (state10 = pose7 | a | b | snapped, dmvio_hip_init_lm.h).
 *
 *   lm_batch_create   a batch of one context with max_windows (in [1, 65535]) LM records of its own; the context's single record is not touched by the batched call.
 *   track_frame_batch W in [0, max_windows] windows; W == 0 returns 0 and counts nothing.  Per window, in: the arguments of resident_track_frame (levels[k] = level k of
 *                     n_levels in [1, the context's levels]; the count may differ from window to window), state_slot: which of the batch's records the window reads and
 *                     writes, state_in10: the incoming state, or NULL to continue from record state_slot (refused while that record is empty).  Out: state_out10
 *                     (required), res3_levels (3 floats per level) and iterations_levels (one int per level), which may be NULL, the trace (trace_d == NULL: none; the
 *                     record layout and the capacity rule of dmvio_hip_init_lm.h), and snapped of the outgoing state.  Returns 0, or < 0 on failure.
 *                     Work per call, whatever W, the level counts and the iteration counts: 1 launch, at most 1 upload (the problem records and the states that came in;
 *                     records equal to what the device holds are not sent again, so a call with unchanged records and every state_in10 NULL uploads nothing), 1 download
 *                     (the W records, the per-level outs and the traces in one copy) and 1 wait.
 *   lm_batch_last_work launches, uploads, downloads and waits of the batch's last track_frame_batch (any pointer may be NULL).  A refused call counts nothing and leaves
 *                     the figures as they were.
 *
 * A refused call is refused as a whole, before anything is enqueued: handles, the batch's records and all outputs stay untouched, and the message names the window.  Refused
 * are: a NULL batch, W outside [0, max_windows], a NULL window array; per window a NULL level array or handle, n_levels out of range, a handle of another context than the
 * batch's, a level handle named twice anywhere in the call, state_slot outside [0, max_windows) or named by two windows, state_out10 == NULL, and everything
 * resident_track_frame refuses, by the same rules: no resident set, a lower level without a parent table or with a parent out of range, any point outside
 * [2, w_lvl - 3) x [2, h_lvl - 3), max_iterations outside [0, 64], a trace without room, a slot out of range, a level whose loop needs more LDS than the device allows a
 * workgroup beside this kernel's own. */
typedef struct dmvio_hip_initializer_lm_batch dmvio_hip_initializer_lm_batch;
dmvio_hip_initializer_lm_batch* dmvio_hip_initializer_lm_batch_create(dmvio_hip_ctx* ctx, int max_windows);
void dmvio_hip_initializer_lm_batch_destroy(dmvio_hip_initializer_lm_batch* b);

typedef struct dmvio_hip_initializer_lm_window {
  /* in: exactly the arguments of dmvio_hip_initializer_resident_track_frame, per window */
  dmvio_hip_initializer* const* levels;
  int n_levels;
  int first_slot, new_slot;
  const double* Ki9_levels;
  const float* fxfycxcy_levels;
  float alphaW, alphaK, regWeight, couplingWeight;
  double priorY, priorX;
  const float* wM8;
  int fix_affine;
  const int* max_iterations;
  int state_slot;
  const double* state_in10;
  /* out */
  double* state_out10;
  float* res3_levels;
  int* iterations_levels;
  int trace_capacity;
  double* trace_d;
  float* trace_f;
  int* trace_records;
  int snapped;
} dmvio_hip_initializer_lm_window;

int dmvio_hip_initializer_resident_track_frame_batch(dmvio_hip_initializer_lm_batch* b, int W, dmvio_hip_initializer_lm_window* win);
int dmvio_hip_initializer_lm_batch_last_work(dmvio_hip_initializer_lm_batch* b, int* launches, int* uploads, int* downloads, int* waits);

#ifdef __cplusplus
}
#endif
#endif
