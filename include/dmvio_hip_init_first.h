/* CoarseInitializer::setFirst on the device: an extension of the C ABI of libdmvio_hip.so (dmvio_hip.h), in a header of its own.  Include it beside dmvio_hip.h and
 * dmvio_hip_init_resident.h; the entry points live in the same library and take the same handles. */
#ifndef DMVIO_HIP_INIT_FIRST_H
#define DMVIO_HIP_INIT_FIRST_H
#include "dmvio_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* What creates the initializer's point sets — CoarseInitializer::setFirst (CoarseInitializer.cpp:804-889) and makeNN (:1001-1078) — on a frame that is resident in a slot:
 * the coarse selector of the levels >= 1 (makePixelStatus, PixelSelector.h:199-253, with gridMaxSelection, :40-196), the raster-ordered point lists (:834-872), the two
 * nearest-neighbour searches, and the hand-over into the resident state of dmvio_hip_init_resident.h without a point value crossing PCIe in the upload direction.
 *   init_first_create   the handle owns the device scratch, sized from the context's image size: a byte map per level, the compacted lists, the neighbour and parent tables.
 *   make_pixel_status   makePixelStatus on dIp[lvl] of the frame in `slot`.  *sparsity_factor is in/out: it replaces the reference's global sparsityFactor (settings.cpp:232,
 *                       initial value 5), which survives from level to level and from call to call; the library holds no copy of it.  The recursion is host code in rounds:
 *                       one select launch and one 4-byte count download per round, at most recs_left + 1 rounds.  *n_good: the return value; map_out_host (may be NULL):
 *                       w_lvl * h_lvl bytes, 0 / 1.  The map of every round, every numGood, the (pot, THFac) trace and the final factor are the reference's, bit for bit.
 *   get_passes          (pot, THFac, numGood) of every round of the last make_pixel_status call (of set_first: of its last level); returns the number of rounds.
 *   make_nn             makeNN's two searches for one level on caller-given host arrays: the ten nearest points of the level (neighbours10, n x 10) and the nearest point of
 *                       the level above for the query (u * 0.5f - 0.25f, v * 0.5f - 0.25f) (parent, n).  n_up == 0 with NULL upper arrays marks the top level: parent is
 *                       all -1.  v (and v_up) must be non-decreasing in the index — raster order, which the search's early end relies on — and every value finite.
 *   set_first           the whole of setFirst for the frame in `slot`, into the L handles ini[0 .. L-1] (level l = ini[l]).  Level 0 runs through `sel`
 *                       (PixelSelector::makeMaps, recursions 1, thFactor 2): its potential is set to 3 for the call and restored afterwards, because the reference uses a
 *                       fresh local PixelSelector; the selector's last-selection state (map, lists, passes, counts) is overwritten.  Levels 1 .. L-1 run make_pixel_status.
 *                       densities: L floats, NULL = the reference's {0.03, 0.05, 0.15, 0.5, 1} (L <= 5), each times w[0] * h[0] in float.  Per point: u = (float)(x + 0.1)
 *                       and v likewise (the addition in double, :841-842), idepth = iR = 1, isGood = 1, energy = 0, lastHessian = 0, outlierTH = outlierTH_per_point (the
 *                       reference: patternNum * setting_outlierTH; its sumGrad2 loop is dead code and is not built), my_type = the level-0 map value, 1 elsewhere.
 *                       n_points (may be NULL): L counts.  After the call every ini[l] is in the state dmvio_hip_initializer_set_resident leaves when given those arrays,
 *                       bit for bit.  The sweep schedule and the children lists are built on the host from ONE download per level (the point list and both tables) and
 *                       are the one upload per level; no point value is uploaded.
 *   get_level           the point list of level lvl of the last set_first: u, v, my_type (floats, FullSystem::initializeFromInitializer reads it at :1597), neighbours10,
 *                       parent (-1 on the top level); each pointer may be NULL.  Returns the point count.  A host copy: no device work.
 *   last_work           launches, uploads, downloads and stream waits of the last make_pixel_status / make_nn / set_first call (level 0's makeMaps not included).
 * Neighbours.  Pnt::neighboursDist and ::parentDist are NOT built: the reference writes them (:1043-1050, :1060) and nothing in it ever reads them.
 * The reference's index sets cannot be matched: nanoflann accepts a candidate only when dist < worstDist (nanoflann.h:1232), so among points tied at the tenth distance the
 * winner is whichever its KD-tree visits first, and with points at integer pixels + 0.1 such ties are the rule.  The library's rule is its own: the ten smallest by
 * (float distance, index) in lexicographic order, the point itself included at distance 0 as in the reference, nearest first; the parent is the smallest
 * (distance, index) of the level above.  The distance is FLANNPointcloud's (CoarseInitializer.h:177-182) in float without contraction: d0 = q0 - u, d1 = q1 - v,
 * d0 * d0 + d1 * d1.  Against the reference this guarantees what is well defined: the same ten distances bit for bit, and a set that is a valid 10-NN set under that metric.
 * optReg's medians, and hence the trajectory, can differ from an all-CPU run at tied points; a caller who needs the reference's tie choice keeps makeNN on the host and calls
 * dmvio_hip_initializer_set_resident.
 * All calls run under the context's lock on the context's stream.
 * Each call is refused as a whole, with a message and with every initializer handle untouched: a NULL handle or handles of different contexts; a slot or level out of range;
 * L different from the context's level count; make_nn with n < 10, n_up < 0, a v that decreases, or a value that is not finite; in set_first — where the selection runs in the
 * handle's scratch first, so nothing of an initializer handle is written before every level has been checked — a level whose point count exceeds its handle's capacity or
 * set_resident's LDS limit, or a level with fewer than 10 points (the reference reads uninitialised result slots there; that case is outside its contract). */
typedef struct dmvio_hip_init_first dmvio_hip_init_first;
dmvio_hip_init_first* dmvio_hip_init_first_create(dmvio_hip_ctx* ctx);
void dmvio_hip_init_first_destroy(dmvio_hip_init_first* first);
int dmvio_hip_init_first_make_pixel_status(dmvio_hip_init_first* first, int slot, int lvl, float desired_density, int recs_left, float th_factor, int* sparsity_factor,
                                           int* n_good, unsigned char* map_out_host);
int dmvio_hip_init_first_get_passes(dmvio_hip_init_first* first, int max_passes, int* pot, float* th_factor, int* n_good);
int dmvio_hip_init_first_make_nn(dmvio_hip_init_first* first, int n, const float* u, const float* v, int n_up, const float* u_up, const float* v_up, int* neighbours10,
                                 int* parent);
int dmvio_hip_initializer_set_first(dmvio_hip_init_first* first, dmvio_hip_pixel_selector* sel, int slot, const float* B_lut256, int L, dmvio_hip_initializer* const* ini,
                                    const float* densities, float outlierTH_per_point, int* sparsity_factor, int* n_points);
int dmvio_hip_init_first_get_level(dmvio_hip_init_first* first, int lvl, float* u, float* v, float* my_type, int* neighbours10, int* parent);
int dmvio_hip_init_first_last_work(dmvio_hip_init_first* first, int* launches, int* uploads, int* downloads, int* waits);

#ifdef __cplusplus
}
#endif
#endif
