// The resident state a handle carries behind dmvio_hip_initializer::resident, shared by the unit that owns it (capi_init_resident.hip: the per-point passes) and the unit that
// runs trackFrame's LM loop on it (capi_init_lm.hip).  Only touched under the context's lock.
#pragma once
#include "init_handle.h"

// One slab holds the point set: [static part | dynamic part].  The upload of set_resident covers the static part and the head of the dynamic one (the fields the caller
// gives); the rest starts zeroed.  get_state downloads the dynamic part.  The pinned side keeps the host copy of (u, v) the range check of calc reads.
struct DmvInitResidentLayout {   // byte offsets into the slab
  size_t o_u, o_v, o_oth, o_nb, o_parent, o_order, o_lbegin, o_cbegin, o_children;                                           // static
  size_t o_idepth, o_iR, o_lh, o_energy, o_good, up_end, o_idn, o_en_new, o_maxstep, o_lh_new, o_jb[2], o_good_new, total;   // dynamic; up_end: where the upload stops
};
struct DmvInitResident : DmvInitResidentLayout {
  bool live = false;
  int n = 0, levels = 0, n_listed = 0, max_parent = -1, cur = 0;   // cur: which of the two JbBuffers is JbBuffer, the other being JbBuffer_new
  bool has_parent = false;
  DmvSlab st;       // the point set
  DmvSlab io;       // [what a calc downloads: IN_PART sums, 3 calcEC sums, the outside count | partials of the evaluation | partials of calcEC]
  DmvWork work;
  bool work_closed = true;
  size_t lds_limit = 0;
  float* f(size_t off) const { return st.dev<float>(off); }
  int* i(size_t off) const { return st.dev<int>(off); }
  unsigned char* b(size_t off) const { return st.dev<unsigned char>(off); }
};
enum { RES_OUT_FLOATS = 128, RES_EC = dmv::IN_PART, RES_COUNT = dmv::IN_PART + 3, RES_DOWN = dmv::IN_PART + 4 };
// bytes of LDS the ordered sweeps need for n points: iR and isGood of the level
static inline size_t resSweepLds(int n) { return (5 * (size_t)n + 3) & ~(size_t)3; }
