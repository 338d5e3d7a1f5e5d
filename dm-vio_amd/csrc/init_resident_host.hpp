// What the resident initializer works out on the host, once per point set (dmvio_hip_initializer_set_resident, dmvInitResidentAdopt): its two static tables and where
// the arrays lie in the slab.  No HIP call and no include of the project's: compiles under a plain host compiler (tests/init_sweep_harness.cpp).
//
// CoarseInitializer::optReg (CoarseInitializer.cpp:671-704) and the top-level branch of resetPoints (:901-916) are in-place loops: point i reads iR / isGood of its ten
// neighbours, of which those with a lower index have been rewritten by the same loop and those with a higher index have not.  The neighbour table is fixed for the life of
// a point set (makeNN runs once, in setFirst), so that order is a static schedule.  With the relation "i names j or j names i" (-1 and self ignored),
//     level(i) = 1 + max level(j) over adjacent j < i, or 0 if there is none,
// two adjacent points never share a level, a point's lower-index adjacent points all sit on lower levels and its higher-index ones on higher levels.  Executing the levels
// in order — every point of a level from the state the levels before it left — therefore gives the serial loop's result for ANY per-point body that reads only the point and
// its neighbours and writes only the point, whatever isGood is at the time.
#pragma once
#include <algorithm>
#include <vector>

// The levels as a CSR: order[level_begin[l] .. level_begin[l + 1]) are the points of level l in ascending index; level_begin has (levels + 1) entries, one entry (0) for
// n == 0.  neighbours10: 10 entries per point, each -1 or in [0, n) (the caller has checked).  Returns the number of levels.
static inline int initSweepSchedule(int n, const int* neighbours10, std::vector<int>& level_begin, std::vector<int>& order) {
  std::vector<int> level((size_t)std::max(n, 0), 0);
  // an asymmetric pair (j names i, i does not name j) binds like a symmetric one: the later of the two must wait for the earlier.  `need[i]` collects, while the lower
  // endpoints pass by, the level the higher endpoint i needs at least.
  std::vector<int> need((size_t)std::max(n, 0), 0);
  int levels = 0;
  for (int i = 0; i < n; i++) {
    int l = need[i];
    for (int k = 0; k < 10; k++) {
      const int j = neighbours10[10 * (size_t)i + k];
      if (j < 0 || j == i) continue;
      if (j < i) l = std::max(l, level[j] + 1);
    }
    level[i] = l;
    for (int k = 0; k < 10; k++) {
      const int j = neighbours10[10 * (size_t)i + k];
      if (j > i) need[j] = std::max(need[j], l + 1);
    }
    levels = std::max(levels, l + 1);
  }
  // (a lower point j that names i only from ITS row reaches i through need[i] above; a lower point j that i names is read directly: both directions of the relation)
  level_begin.assign((size_t)levels + 1, 0);
  for (int i = 0; i < n; i++) level_begin[(size_t)level[i] + 1]++;
  for (int l = 0; l < levels; l++) level_begin[(size_t)l + 1] += level_begin[l];
  order.assign((size_t)std::max(n, 0), 0);
  std::vector<int> at(level_begin.begin(), level_begin.end() - 1);
  for (int i = 0; i < n; i++) order[(size_t)at[level[i]]++] = i;   // ascending i inside a level
  return levels;
}

// The children of every parent of the level above, in ascending child index — the order CoarseInitializer::propagateUp (:726-734) adds them in.  parent: n_src entries in
// [0, n_dst) (the caller has checked).  child_begin: n_dst + 1 entries; children: n_src.
static inline void initChildLists(int n_src, const int* parent, int n_dst, std::vector<int>& child_begin, std::vector<int>& children) {
  child_begin.assign((size_t)std::max(n_dst, 0) + 1, 0);
  for (int i = 0; i < n_src; i++) child_begin[(size_t)parent[i] + 1]++;
  for (int p = 0; p < n_dst; p++) child_begin[(size_t)p + 1] += child_begin[p];
  children.assign((size_t)std::max(n_src, 0), 0);
  std::vector<int> at(child_begin.begin(), child_begin.end() - 1);
  for (int i = 0; i < n_src; i++) children[(size_t)at[parent[i]]++] = i;
}

// One slab holds the point set: [static part | dynamic part], byte offsets.  The upload of set_resident covers the static part and the head of the dynamic one (the fields
// the caller gives, up to up_end); the rest starts zeroed.  get_state downloads the dynamic part.  The four tables the host builds — order, level_begin, child_begin,
// children — lie back to back in front of the dynamic part: dmvInitResidentAdopt, whose point arrays are written on the device, uploads [o_order, o_idepth) as one copy.
struct DmvInitResidentLayout {
  size_t o_u, o_v, o_oth, o_nb, o_parent, o_order, o_lbegin, o_cbegin, o_children;                                           // static
  size_t o_idepth, o_iR, o_lh, o_energy, o_good, up_end, o_idn, o_en_new, o_maxstep, o_lh_new, o_jb[2], o_good_new, total;   // dynamic
};
// n points, `levels` sweep levels, n_listed parents listed.  CURSOR: DmvCursor (batch_slab.hpp), the one alignment rule of the slabs; a parameter so that this header
// needs nothing but itself.
template <class CURSOR>
static inline DmvInitResidentLayout initResidentLayout(int n, int levels, int n_listed) {
  CURSOR L;
  DmvInitResidentLayout N;
  N.o_u = L.template take<float>(n); N.o_v = L.template take<float>(n); N.o_oth = L.template take<float>(n); N.o_nb = L.template take<int>(10 * (size_t)n); N.o_parent = L.template take<int>(n);
  N.o_order = L.template take<int>(n); N.o_lbegin = L.template take<int>((size_t)levels + 1); N.o_cbegin = L.template take<int>((size_t)n_listed + 1); N.o_children = L.template take<int>(n);
  N.o_idepth = L.template take<float>(n); N.o_iR = L.template take<float>(n); N.o_lh = L.template take<float>(n); N.o_energy = L.template take<float>(2 * (size_t)n); N.o_good = L.template take<unsigned char>(n);
  N.up_end = L.bytes();
  N.o_idn = L.template take<float>(n); N.o_en_new = L.template take<float>(2 * (size_t)n); N.o_maxstep = L.template take<float>(n); N.o_lh_new = L.template take<float>(n);
  N.o_jb[0] = L.template take<float>(10 * (size_t)n); N.o_jb[1] = L.template take<float>(10 * (size_t)n); N.o_good_new = L.template take<unsigned char>(n);
  N.total = L.bytes();
  return N;
}
