// The two host tables of the resident initializer (dm-vio_amd/csrc/init_resident_host.hpp) as a program of their own (tests/test_init_resident_cpu.py compiles it with g++
// alone, with AddressSanitizer and UBSan where their runtimes exist): for hand-made graphs and for every graph in the files named on the command line, executing the levels
// of initSweepSchedule in order — every point of a level from the state the levels before it left — equals the serial in-place loop, for two bodies shaped like optReg's and
// like the top-level resetPoints'; initChildLists lists every parent's children in ascending index; and initResidentLayout puts every array of the point set's slab on a
// 256-byte boundary, in declaration order, with the four host-built tables back to back in front of the dynamic part (the one copy of dmvInitResidentAdopt).
// A graph file: int32 n, then 10 n int32 neighbours (-1 = none), then n int32 parents (-1 throughout = none).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
static int failmsg(const std::string&) { return -2; }   // (batch_slab.hpp words refusals through it; none is reached here)
#include "batch_slab.hpp"   // DmvCursor, the cursor the library lays the slab out with
#include "init_resident_host.hpp"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

struct State { std::vector<float> x, y; std::vector<unsigned char> good; };

// what the body of point i writes, from the state it sees: (new x, new good)
static void bodyMedian(const State& s, const int* nb, int i, float* x, unsigned char* good) {
  *x = s.x[i]; *good = s.good[i];
  if (!s.good[i]) return;
  float v[10]; int n = 0;
  for (int k = 0; k < 10; k++) { const int j = nb[10 * i + k]; if (j == -1 || !s.good[j]) continue; v[n++] = s.x[j]; }
  if (n > 2) { std::nth_element(v, v + n / 2, v + n); *x = 0.2f * s.y[i] + 0.8f * v[n / 2]; }
}
static void bodyRevive(const State& s, const int* nb, int i, float* x, unsigned char* good) {
  *x = s.x[i]; *good = s.good[i];
  if (s.good[i]) return;
  float sum = 0, cnt = 0;
  for (int k = 0; k < 10; k++) { const int j = nb[10 * i + k]; if (j == -1 || !s.good[j]) continue; sum += s.x[j]; cnt += 1; }
  if (cnt > 0) { *good = 1; *x = sum / cnt; }
}
typedef void (*Body)(const State&, const int*, int, float*, unsigned char*);

static State makeState(int n, unsigned seed) {
  State s; s.x.resize(n); s.y.resize(n); s.good.resize(n);
  for (int i = 0; i < n; i++) {
    seed = seed * 1664525u + 1013904223u; s.x[i] = (float)(seed >> 8) / 16777216.0f * 3.0f;
    seed = seed * 1664525u + 1013904223u; s.y[i] = (float)(seed >> 8) / 16777216.0f * 3.0f;
    seed = seed * 1664525u + 1013904223u; s.good[i] = (seed >> 16) % 5 != 0;
  }
  return s;
}

static void checkGraph(const char* name, int n, const std::vector<int>& nb, int want_levels = -1, int want_widest = -1) {
  std::vector<int> lb, order;
  const int levels = initSweepSchedule(n, nb.data(), lb, order);
  CHECK((int)lb.size() == levels + 1 && lb[0] == 0 && lb[levels] == n && (int)order.size() == n, "%s: CSR shape", name);
  if (want_levels >= 0) CHECK(levels == want_levels, "%s: %d levels, expected %d", name, levels, want_levels);
  std::vector<int> level(n, -1);
  int widest = 0;
  for (int l = 0; l < levels; l++) {
    CHECK(lb[l + 1] > lb[l], "%s: empty level %d", name, l);
    widest = std::max(widest, lb[l + 1] - lb[l]);
    for (int k = lb[l]; k < lb[l + 1]; k++) {
      CHECK(order[k] >= 0 && order[k] < n && level[order[k]] == -1, "%s: order is no permutation", name);
      if (k > lb[l]) CHECK(order[k] > order[k - 1], "%s: level %d not ascending", name, l);
      level[order[k]] = l;
    }
  }
  if (want_widest >= 0) CHECK(widest == want_widest, "%s: widest level %d, expected %d", name, widest, want_widest);
  for (int i = 0; i < n; i++)
    for (int k = 0; k < 10; k++) {
      const int j = nb[10 * i + k];
      if (j < 0 || j == i) continue;
      CHECK((j < i) == (level[j] < level[i]) && level[j] != level[i], "%s: points %d (level %d) and %d (level %d) are adjacent", name, i, level[i], j, level[j]);
    }
  const Body bodies[2] = {bodyMedian, bodyRevive};
  for (int b = 0; b < 2; b++)
    for (unsigned seed = 1; seed <= 3; seed++) {
      State serial = makeState(n, seed * 77u + b), lev = serial;
      for (int i = 0; i < n; i++) { float x; unsigned char g; bodies[b](serial, nb.data(), i, &x, &g); serial.x[i] = x; serial.good[i] = g; }
      for (int l = 0; l < levels; l++) {
        // every point of the level from the state before the level: what lanes of one wavefront between two barriers see
        std::vector<float> x(lb[l + 1] - lb[l]); std::vector<unsigned char> g(x.size());
        for (int k = lb[l]; k < lb[l + 1]; k++) bodies[b](lev, nb.data(), order[k], &x[k - lb[l]], &g[k - lb[l]]);
        for (int k = lb[l]; k < lb[l + 1]; k++) { lev.x[order[k]] = x[k - lb[l]]; lev.good[order[k]] = g[k - lb[l]]; }
      }
      CHECK(n == 0 || (memcmp(serial.x.data(), lev.x.data(), sizeof(float) * n) == 0 && memcmp(serial.good.data(), lev.good.data(), n) == 0),
            "%s: body %d, seed %u: the levels in order differ from the serial loop", name, b, seed);
    }
}

static void checkChildren(const char* name, int n_src, const std::vector<int>& parent, int n_dst) {
  std::vector<int> cb, ch;
  initChildLists(n_src, parent.data(), n_dst, cb, ch);
  CHECK((int)cb.size() == n_dst + 1 && cb[0] == 0 && cb[n_dst] == n_src && (int)ch.size() == n_src, "%s: CSR shape", name);
  std::vector<int> seen(n_src, 0);
  for (int p = 0; p < n_dst; p++)
    for (int k = cb[p]; k < cb[p + 1]; k++) {
      CHECK(parent[ch[k]] == p, "%s: child %d listed under parent %d", name, ch[k], p);
      if (k > cb[p]) CHECK(ch[k] > ch[k - 1], "%s: children of %d not ascending", name, p);
      seen[ch[k]]++;
    }
  for (int i = 0; i < n_src; i++) CHECK(seen[i] == 1, "%s: child %d listed %d times", name, i, seen[i]);
}

static void checkLayout(int n, int levels, int n_listed) {
  const DmvInitResidentLayout N = initResidentLayout<DmvCursor>(n, levels, n_listed);
  char name[64];
  snprintf(name, sizeof(name), "layout n=%d levels=%d listed=%d", n, levels, n_listed);
  const size_t F = sizeof(float) * (size_t)n, I = sizeof(int) * (size_t)n;
  // every array in declaration order: offset and bytes
  const struct { size_t off, bytes; } part[] = {
      {N.o_u, F}, {N.o_v, F}, {N.o_oth, F}, {N.o_nb, 10 * I}, {N.o_parent, I}, {N.o_order, I}, {N.o_lbegin, sizeof(int) * ((size_t)levels + 1)},
      {N.o_cbegin, sizeof(int) * ((size_t)n_listed + 1)}, {N.o_children, I}, {N.o_idepth, F}, {N.o_iR, F}, {N.o_lh, F}, {N.o_energy, 2 * F}, {N.o_good, (size_t)n},
      {N.o_idn, F}, {N.o_en_new, 2 * F}, {N.o_maxstep, F}, {N.o_lh_new, F}, {N.o_jb[0], 10 * F}, {N.o_jb[1], 10 * F}, {N.o_good_new, (size_t)n}};
  const int parts = (int)(sizeof(part) / sizeof(part[0]));
  CHECK(N.o_u == 0, "%s: the slab does not start with u", name);
  for (int k = 0; k < parts; k++) {
    CHECK(part[k].off % 256 == 0, "%s: array %d at %zu is not 256-byte aligned", name, k, part[k].off);
    if (k) CHECK(part[k].off >= part[k - 1].off + part[k - 1].bytes, "%s: array %d at %zu starts inside array %d (%zu + %zu)", name, k, part[k].off, k - 1, part[k - 1].off, part[k - 1].bytes);
  }
  CHECK(N.up_end % 256 == 0 && N.total % 256 == 0, "%s: up_end %zu or total %zu is not 256-byte aligned", name, N.up_end, N.total);
  // [o_order, o_idepth) is order | level_begin | child_begin | children, each padded to the boundary, and nothing else
  const size_t pad = 255;
  CHECK(N.o_lbegin == N.o_order + ((I + pad) & ~pad), "%s: level_begin does not follow order", name);
  CHECK(N.o_cbegin == N.o_lbegin + ((part[6].bytes + pad) & ~pad), "%s: child_begin does not follow level_begin", name);
  CHECK(N.o_children == N.o_cbegin + ((part[7].bytes + pad) & ~pad), "%s: children does not follow child_begin", name);
  CHECK(N.o_idepth == N.o_children + ((I + pad) & ~pad), "%s: the dynamic part does not follow children", name);
  CHECK(N.up_end >= N.o_good + (size_t)n && N.up_end <= N.o_idn, "%s: up_end %zu outside [end of isGood %zu, idepth_new %zu]", name, N.up_end, N.o_good + (size_t)n, N.o_idn);
  CHECK(N.total >= N.o_good_new + (size_t)n, "%s: total %zu does not cover isGood_new (%zu + %d)", name, N.total, N.o_good_new, n);
}

int main(int argc, char** argv) {
  for (int n : {0, 1, 63, 64, 65})
    for (int levels : {1, 3})
      for (int n_listed : {0, 1, n}) checkLayout(n, levels, n_listed);
  {   // a chain i -> i - 1: n levels of one point
    const int n = 300;
    std::vector<int> nb(10 * n, -1);
    for (int i = 1; i < n; i++) nb[10 * i + 3] = i - 1;
    checkGraph("chain", n, nb, n, 1);
  }
  {   // the same chain named from the other end only (i -> i + 1): the relation is symmetrised
    const int n = 70;
    std::vector<int> nb(10 * n, -1);
    for (int i = 0; i + 1 < n; i++) nb[10 * i] = i + 1;
    checkGraph("chain named forward", n, nb, n, 1);
  }
  {   // all independent: one level of width n
    const int n = 200;
    std::vector<int> nb(10 * n, -1);
    for (int i = 0; i < n; i++) nb[10 * i + 5] = i;   // self is ignored
    checkGraph("independent", n, nb, 1, n);
  }
  {   // an asymmetric pair: 5 names 2, 2 names nobody; and 1 names 4, 4 names nobody
    const int n = 6;
    std::vector<int> nb(10 * n, -1);
    nb[10 * 5 + 0] = 2; nb[10 * 1 + 9] = 4;
    checkGraph("asymmetric pair", n, nb, 2, 4);
  }
  { std::vector<int> nb; checkGraph("n = 0", 0, nb, 0, 0); }
  { std::vector<int> nb(10, -1); nb[0] = 0; checkGraph("n = 1", 1, nb, 1, 1); }
  {   // a dense pseudo-random graph with duplicates in a row
    const int n = 500;
    std::vector<int> nb(10 * n, -1);
    unsigned s = 12345;
    for (int k = 0; k < 10 * n; k++) { s = s * 1664525u + 1013904223u; const int near = (int)((s >> 10) % 41) - 20 + k / 10; if ((s >> 4) % 7 && near >= 0 && near < n) nb[k] = near; }
    checkGraph("random band", n, nb);
  }
  checkChildren("no children", 0, std::vector<int>(), 4);
  checkChildren("one parent", 5, std::vector<int>(5, 0), 1);
  { std::vector<int> p = {3, 0, 3, 1, 0, 3, 5}; checkChildren("gaps", 7, p, 7); }
  int files = 0;
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { printf("FAILED: cannot open %s\n", argv[a]); return 2; }
    int n = 0;
    if (fread(&n, sizeof(int), 1, f) != 1 || n < 0) { printf("FAILED: %s: no point count\n", argv[a]); return 2; }
    std::vector<int> nb(10 * (size_t)n), parent((size_t)n);
    if (fread(nb.data(), sizeof(int), nb.size(), f) != nb.size() || fread(parent.data(), sizeof(int), parent.size(), f) != parent.size()) { printf("FAILED: %s: short\n", argv[a]); return 2; }
    fclose(f);
    checkGraph(argv[a], n, nb);
    if (n && parent[0] >= 0) checkChildren(argv[a], n, parent, 1 + *std::max_element(parent.begin(), parent.end()));
    files++;
  }
  if (g_fail) { printf("%d check(s) FAILED\n", g_fail); return 1; }
  printf("ok init_sweep_harness: hand-made graphs, the slab layouts and %d graph file(s)\n", files);
  return 0;
}
