// C ABI of setFirst on the device (include/dmvio_hip_init_first.h): the coarse selector of the levels >= 1, the raster-ordered point lists, makeNN's two searches and the
// hand-over into the resident initializer (capi_init_resident.hip: dmvInitResidentAdopt).  Level 0's selection is the pixel selector's (capi_select.hip).
#include <vector>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <algorithm>
#include "../../include/dmvio_hip_init_first.h"
#include "init_handle.h"
#include "init_first_kernels.hpp"

using namespace dmv;

struct FirstLevel {
  int w = 0, h = 0, ntiles = 0, n = 0;
  unsigned char* d_map = nullptr;   // w * h bytes
  int* d_tiles = nullptr;           // ntiles
  DmvSlab pts;                      // [u | v | my_type | neighbours10 | parent] of the level's n points, packed for n once n is known; sized for every pixel of the window
  size_t o_u = 0, o_v = 0, o_type = 0, o_nb = 0, o_parent = 0, bytes = 0;
  void layout(int n_) {
    DmvCursor L;
    n = n_;
    o_u = L.take<float>(n); o_v = L.take<float>(n); o_type = L.take<float>(n); o_nb = L.take<int>(10 * (size_t)n); o_parent = L.take<int>(n);
    bytes = L.bytes();
  }
};
enum { FIRST_CNT_GOOD = 0, FIRST_CNT_N = 1, FIRST_CNT_INTS = 16 };   // the counter block: numGood of a select round, then the point count of every level

struct dmvio_hip_init_first {
  dmvio_hip_ctx* ctx = nullptr;
  int levels = 0;
  FirstLevel lv[DMV_MAX_LEVELS];
  DmvSlab cnt;    // FIRST_CNT_INTS ints
  DmvSlab nn;     // make_nn's arrays: [u | v | u_up | v_up | neighbours10 | parent], grown to the call
  DmvWork work;
  bool have_first = false;   // get_level has something to return
  std::vector<int> pass_pot, pass_good;
  std::vector<float> pass_th;
};

static void firstRelease(dmvio_hip_init_first* F) {
  for (FirstLevel& V : F->lv) { if (V.d_map) hipFree(V.d_map); if (V.d_tiles) hipFree(V.d_tiles); V.pts.release(); }
  F->cnt.release(); F->nn.release();
}
static inline dim3 firstGrid(int n) { return dim3((unsigned)std::max(1, (n + 255) / 256)); }
#define FIRST_HEAD(F, who)                                                      \
  if (!(F)) return failmsg(who ": null init_first handle");                     \
  HIPCHK(hipSetDevice((F)->ctx->device));                                       \
  dmvio_hip_ctx* c = (F)->ctx;                                                  \
  std::lock_guard<std::mutex> lk(c->mu);                                        \
  hipStream_t s = c->stream;                                                    \
  (void)s

// makePixelStatus (PixelSelector.h:199-253) on level lvl of the frame in `slot`, into the level's map; its recursion is this loop, every expression typed as there
static int firstPixelStatus(dmvio_hip_init_first* F, int slot, int lvl, float desiredDensity, int recsLeft, float THFac, int* sparsityFactor_io, int* numGood) {
  dmvio_hip_ctx* c = F->ctx;
  hipStream_t s = c->stream;
  FirstLevel& V = F->lv[lvl];
  if (lvl == 0) { if (int r = dmv_ensure_row_major_locked(c, slot)) return r; }
  const float* I = c->frames.levelPtr(slot, lvl);
  int sparsityFactor = *sparsityFactor_io;
  F->pass_pot.clear(); F->pass_good.clear(); F->pass_th.clear();
  int* d_good = F->cnt.dev<int>(0) + FIRST_CNT_GOOD;
  for (;;) {
    if (sparsityFactor < 1) sparsityFactor = 1;
    const int pot = sparsityFactor;
    const int ncx = std::max(0, (V.w - 2) / pot), ncy = std::max(0, (V.h - 2) / pot);   // cells start at 1 and step by pot while < w - pot
    HIPCHK(hipMemsetAsync(V.d_map, 0, (size_t)V.w * V.h, s));
    HIPCHK(hipMemsetAsync(d_good, 0, sizeof(int), s));
    if (ncx * ncy > 0) {
      hipLaunchKernelGGL(k_first_grid_select, firstGrid(ncx * ncy), dim3(256), 0, s, I, V.w, V.h, pot, THFac, ncx, ncy, V.d_map, d_good);
      HIPCHK(hipGetLastError());
      F->work.launches++;
    }
    if (int r = F->cnt.download(s, sizeof(int) * FIRST_CNT_GOOD, sizeof(int))) return r;
    if (int r = F->cnt.wait(s)) return r;
    const int numGoodPoints = F->cnt.host<int>(0)[FIRST_CNT_GOOD];
    F->pass_pot.push_back(pot); F->pass_th.push_back(THFac); F->pass_good.push_back(numGoodPoints);
    const float quotia = numGoodPoints / (float)(desiredDensity);
    int newSparsity = (sparsityFactor * sqrtf(quotia)) + 0.7f;
    if (newSparsity < 1) newSparsity = 1;
    const float oldTHFac = THFac;
    if (newSparsity == 1 && sparsityFactor == 1) THFac = 0.5;
    const bool done = (abs(newSparsity - sparsityFactor) < 1 && THFac == oldTHFac) || (quotia > 0.8 && 1.0f / quotia > 0.8) || recsLeft == 0;
    sparsityFactor = newSparsity;
    if (done) { *numGood = numGoodPoints; break; }
    recsLeft--;
  }
  *sparsityFactor_io = sparsityFactor;
  return 0;
}

// the flagged window pixels of `map` counted in raster order: tile sums, their scan, the total into the counter block.  The list itself is written by firstCompact once
// the host knows the count.
static int firstCount(dmvio_hip_init_first* F, int lvl, const unsigned char* d_map) {
  FirstLevel& V = F->lv[lvl];
  hipStream_t s = F->ctx->stream;
  hipLaunchKernelGGL(k_first_scanA, dim3(V.ntiles), dim3(256), 0, s, d_map, V.w, V.h, V.d_tiles);
  hipLaunchKernelGGL(k_first_scanB, dim3(1), dim3(256), 0, s, V.d_tiles, V.ntiles, F->cnt.dev<int>(0) + FIRST_CNT_N + lvl);
  HIPCHK(hipGetLastError());
  F->work.launches += 2;
  return 0;
}
static int firstCompact(dmvio_hip_init_first* F, int lvl, const unsigned char* d_map, int n) {
  FirstLevel& V = F->lv[lvl];
  hipStream_t s = F->ctx->stream;
  V.layout(n);
  hipLaunchKernelGGL(k_first_scanC, dim3(V.ntiles), dim3(256), 0, s, d_map, V.w, V.h, (const int*)V.d_tiles, lvl == 0 ? 1 : 0, n, V.pts.dev<float>(V.o_u), V.pts.dev<float>(V.o_v),
                     V.pts.dev<float>(V.o_type));
  HIPCHK(hipGetLastError());
  F->work.launches++;
  return 0;
}
// the ten nearest of the level itself; the nearest of the level above (d_uu NULL: none)
static int firstSearch(dmvio_hip_init_first* F, int n, const float* d_u, const float* d_v, int n_up, const float* d_uu, const float* d_vu, int* d_nb, int* d_parent) {
  hipStream_t s = F->ctx->stream;
  hipLaunchKernelGGL((k_first_knn<10, false>), firstGrid(n), dim3(FIRST_KNN_WG), 0, s, n, d_u, d_v, n, d_u, d_v, d_nb);
  F->work.launches++;
  if (d_uu) {
    hipLaunchKernelGGL((k_first_knn<1, true>), firstGrid(n), dim3(FIRST_KNN_WG), 0, s, n, d_u, d_v, n_up, d_uu, d_vu, d_parent);
    F->work.launches++;
  } else {
    HIPCHK(hipMemsetAsync(d_parent, 0xFF, sizeof(int) * (size_t)n, s));   // -1
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" {

dmvio_hip_init_first* dmvio_hip_init_first_create(dmvio_hip_ctx* ctx) {
  if (!ctx) { failmsg("init_first_create: null context"); return nullptr; }
  HIPCHKP(hipSetDevice(ctx->device));
  dmvio_hip_init_first* F = new dmvio_hip_init_first();
  F->ctx = ctx; F->levels = ctx->levels;
  bool ok = F->cnt.create(sizeof(int) * FIRST_CNT_INTS) == 0;
  for (int l = 0; ok && l < F->levels; l++) {
    FirstLevel& V = F->lv[l];
    V.w = ctx->wl[l]; V.h = ctx->hl[l];
    V.ntiles = (V.w * V.h + FIRST_TILE - 1) / FIRST_TILE;
    const int cap = std::max(V.w - 7, 0) * std::max(V.h - 7, 0);   // setFirst's window
    V.layout(cap);
    ok = hipMalloc((void**)&V.d_map, (size_t)V.w * V.h) == hipSuccess && hipMalloc((void**)&V.d_tiles, sizeof(int) * (size_t)V.ntiles) == hipSuccess && V.pts.create(V.bytes) == 0;
    V.layout(0);
  }
  if (!ok) {
    if (dmv_err().empty()) failmsg("init_first_create: allocation failed");
    firstRelease(F);
    delete F;
    return nullptr;
  }
  F->cnt.work = &F->work; F->nn.work = &F->work;
  for (int l = 0; l < F->levels; l++) F->lv[l].pts.work = &F->work;
  return F;
}
void dmvio_hip_init_first_destroy(dmvio_hip_init_first* F) {
  if (!F) return;
  hipSetDevice(F->ctx->device);
  hipStreamSynchronize(F->ctx->stream);
  firstRelease(F);
  delete F;
}

int dmvio_hip_init_first_make_pixel_status(dmvio_hip_init_first* F, int slot, int lvl, float desired_density, int recs_left, float th_factor, int* sparsity_factor,
                                           int* n_good, unsigned char* map_out_host) {
  FIRST_HEAD(F, "init_first_make_pixel_status");
  if (slot < 0 || slot >= c->n_slots || lvl < 0 || lvl >= F->levels) return failmsg("init_first_make_pixel_status: level / slot out of range");
  if (!sparsity_factor || !n_good) return failmsg("init_first_make_pixel_status: null argument");
  if (!(desired_density > 0.f) || recs_left < 0 || !(th_factor > 0.f)) return failmsg("init_first_make_pixel_status: desired_density and th_factor must be positive, recs_left not negative");
  F->work.clear();
  int sf = *sparsity_factor, ng = 0;
  if (int r = firstPixelStatus(F, slot, lvl, desired_density, recs_left, th_factor, &sf, &ng)) return r;
  if (map_out_host) {
    HIPCHK(c->bounce.d2h(map_out_host, F->lv[lvl].d_map, (size_t)F->lv[lvl].w * F->lv[lvl].h, s));
    HIPCHK(c->bounce.finish(s));
    F->work.downloads++; F->work.waits++;
  }
  *sparsity_factor = sf; *n_good = ng;
  return 0;
}

int dmvio_hip_init_first_get_passes(dmvio_hip_init_first* F, int max_passes, int* pot, float* th_factor, int* n_good) {
  if (!F) return failmsg("init_first_get_passes: null init_first handle");
  std::lock_guard<std::mutex> lk(F->ctx->mu);
  const int n = (int)F->pass_pot.size();
  for (int i = 0; i < n && i < max_passes; i++) {
    if (pot) pot[i] = F->pass_pot[i];
    if (th_factor) th_factor[i] = F->pass_th[i];
    if (n_good) n_good[i] = F->pass_good[i];
  }
  return n;
}

int dmvio_hip_init_first_make_nn(dmvio_hip_init_first* F, int n, const float* u, const float* v, int n_up, const float* u_up, const float* v_up, int* neighbours10,
                                 int* parent) {
  static const char* who = "init_first_make_nn";
  FIRST_HEAD(F, "init_first_make_nn");
  char msg[256];
  if (!u || !v || !neighbours10 || !parent) return failmsg(std::string(who) + ": null array");
  if (n < 10) { snprintf(msg, sizeof(msg), "%s: n = %d: a level needs at least 10 points (the reference reads uninitialised result slots below that)", who, n); return failmsg(msg); }
  if (n_up < 0 || (n_up > 0 && (!u_up || !v_up)) || (n_up == 0 && (u_up || v_up))) return failmsg(std::string(who) + ": n_up > 0 needs both upper arrays, n_up == 0 (the top level) neither");
  for (int k = 0; k < 2; k++) {
    const float *a = k ? u_up : u, *b = k ? v_up : v;
    const int m = k ? n_up : n;
    for (int i = 0; i < m; i++) {
      if (!std::isfinite(a[i]) || !std::isfinite(b[i])) { snprintf(msg, sizeof(msg), "%s: point %d of the %s level is not finite", who, i, k ? "upper" : "lower"); return failmsg(msg); }
      if (i && b[i] < b[i - 1]) { snprintf(msg, sizeof(msg), "%s: v of the %s level decreases at point %d (the points must come in raster order)", who, k ? "upper" : "lower", i); return failmsg(msg); }
    }
  }
  F->work.clear();
  DmvCursor L;
  const size_t o_u = L.take<float>(n), o_v = L.take<float>(n), o_uu = L.take<float>(n_up), o_vu = L.take<float>(n_up), up_end = L.bytes();
  const size_t o_nb = L.take<int>(10 * (size_t)n), o_par = L.take<int>(n);
  if (int r = F->nn.reserve(L.bytes(), L.bytes() + L.bytes() / 2, s)) return r;
  if (int r = F->nn.begin(s)) return r;
  memcpy(F->nn.host<float>(o_u), u, sizeof(float) * (size_t)n); memcpy(F->nn.host<float>(o_v), v, sizeof(float) * (size_t)n);
  if (n_up) { memcpy(F->nn.host<float>(o_uu), u_up, sizeof(float) * (size_t)n_up); memcpy(F->nn.host<float>(o_vu), v_up, sizeof(float) * (size_t)n_up); }
  if (int r = F->nn.upload(s, up_end)) return r;
  if (int r = firstSearch(F, n, F->nn.dev<float>(o_u), F->nn.dev<float>(o_v), n_up, n_up ? F->nn.dev<float>(o_uu) : nullptr, n_up ? F->nn.dev<float>(o_vu) : nullptr,
                          F->nn.dev<int>(o_nb), F->nn.dev<int>(o_par))) return r;
  if (int r = F->nn.download(s, o_nb, L.bytes() - o_nb)) return r;
  if (int r = F->nn.wait(s)) return r;
  memcpy(neighbours10, F->nn.host<int>(o_nb), sizeof(int) * 10 * (size_t)n);
  memcpy(parent, F->nn.host<int>(o_par), sizeof(int) * (size_t)n);
  return 0;
}

int dmvio_hip_initializer_set_first(dmvio_hip_init_first* F, dmvio_hip_pixel_selector* sel, int slot, const float* B_lut256, int L, dmvio_hip_initializer* const* ini,
                                    const float* densities, float outlierTH_per_point, int* sparsity_factor, int* n_points) {
  static const char* who = "initializer_set_first";
  static const float REF_DENSITIES[5] = {0.03f, 0.05f, 0.15f, 0.5f, 1.0f};   // :815 (a float array there)
  if (!F || !sel) return failmsg(std::string(who) + ": null init_first or pixel selector handle");
  if (!ini || !sparsity_factor) return failmsg(std::string(who) + ": null argument");
  HIPCHK(hipSetDevice(F->ctx->device));
  dmvio_hip_ctx* c = F->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  hipStream_t s = c->stream;
  char msg[256];
  if (dmv_selector_ctx(sel) != c) return failmsg(std::string(who) + ": the pixel selector belongs to another context");
  if (L != c->levels) { snprintf(msg, sizeof(msg), "%s: L = %d, the context has %d pyramid levels", who, L, c->levels); return failmsg(msg); }
  for (int l = 0; l < L; l++) {
    if (!ini[l]) { snprintf(msg, sizeof(msg), "%s: the initializer handle of level %d is NULL", who, l); return failmsg(msg); }
    if (ini[l]->ctx != c) { snprintf(msg, sizeof(msg), "%s: the initializer handle of level %d belongs to another context", who, l); return failmsg(msg); }
    for (int k = 0; k < l; k++) if (ini[k] == ini[l]) { snprintf(msg, sizeof(msg), "%s: one initializer handle named for levels %d and %d", who, k, l); return failmsg(msg); }
  }
  if (slot < 0 || slot >= c->n_slots) return failmsg(std::string(who) + ": frame slot out of range");
  if (!densities && L > 5) return failmsg(std::string(who) + ": the reference lists 5 densities; more levels need the caller's");
  if (!densities) densities = REF_DENSITIES;
  F->work.clear();
  F->have_first = false;
  // ---- the selection, in the scratch: level 0 by the selector at potential 3 (a fresh PixelSelector, :810, :818), the others by makePixelStatus
  const int w0 = c->wl[0], h0 = c->hl[0];
  const int saved = dmvio_hip_pixel_selector_get_potential(sel);
  dmvio_hip_pixel_selector_set_potential(sel, 3);
  int nsel = 0;
  const int r0 = dmv_selector_make_maps_locked(sel, slot, B_lut256, densities[0] * w0 * h0, 1, 2.0f, &nsel, nullptr, nullptr);
  dmvio_hip_pixel_selector_set_potential(sel, saved);
  if (r0) return r0;
  if (int r = firstCount(F, 0, dmv_selector_map(sel))) return r;
  int sf = *sparsity_factor;
  for (int l = 1; l < L; l++) {
    int ng = 0;
    if (int r = firstPixelStatus(F, slot, l, densities[l] * w0 * h0, 5, 1.0f, &sf, &ng)) return r;
    if (int r = firstCount(F, l, F->lv[l].d_map)) return r;
  }
  if (int r = F->cnt.download(s, sizeof(int) * FIRST_CNT_N, sizeof(int) * (size_t)L)) return r;
  if (int r = F->cnt.wait(s)) return r;
  int n[DMV_MAX_LEVELS];
  for (int l = 0; l < L; l++) n[l] = F->cnt.host<int>(0)[FIRST_CNT_N + l];
  // ---- every refusal that depends on the selection, before a handle is written
  for (int l = 0; l < L; l++) {
    if (n[l] < 10) { snprintf(msg, sizeof(msg), "%s: level %d has %d points; a level needs at least 10 (the reference reads uninitialised result slots below that)", who, l, n[l]); return failmsg(msg); }
    snprintf(msg, sizeof(msg), "%s: level %d", who, l);
    const std::string tag(msg);
    if (int r = dmvInitResidentCheck(ini[l], n[l], tag.c_str())) return r;
  }
  // ---- the lists, the searches, ONE download per level, one wait
  for (int l = 0; l < L; l++) if (int r = firstCompact(F, l, l == 0 ? dmv_selector_map(sel) : F->lv[l].d_map, n[l])) return r;
  for (int l = 0; l < L; l++) {
    FirstLevel &V = F->lv[l], *U = l + 1 < L ? &F->lv[l + 1] : nullptr;
    if (int r = firstSearch(F, V.n, V.pts.dev<float>(V.o_u), V.pts.dev<float>(V.o_v), U ? U->n : 0, U ? U->pts.dev<float>(U->o_u) : nullptr, U ? U->pts.dev<float>(U->o_v) : nullptr,
                            V.pts.dev<int>(V.o_nb), V.pts.dev<int>(V.o_parent))) return r;
    if (int r = V.pts.download(s, 0, V.bytes)) return r;
  }
  if (int r = F->cnt.wait(s)) return r;
  // ---- the hand-over: schedule and children lists from the host copy, everything per point device to device
  for (int l = 0; l < L; l++) {
    FirstLevel& V = F->lv[l];
    const int* h_nb = V.pts.host<int>(V.o_nb);
    const int* h_par = l + 1 < L ? V.pts.host<int>(V.o_parent) : nullptr;
    for (size_t k = 0; k < 10 * (size_t)V.n; k++) if (h_nb[k] < 0 || h_nb[k] >= V.n) return failmsg(std::string(who) + ": internal: a neighbour index out of range");
    if (h_par) for (int i = 0; i < V.n; i++) if (h_par[i] < 0 || h_par[i] >= F->lv[l + 1].n) return failmsg(std::string(who) + ": internal: a parent index out of range");
    if (int r = dmvInitResidentAdopt(ini[l], V.n, V.pts.dev<float>(V.o_u), V.pts.dev<float>(V.o_v), V.pts.dev<int>(V.o_nb), h_par ? V.pts.dev<int>(V.o_parent) : nullptr,
                                     V.pts.host<float>(V.o_u), V.pts.host<float>(V.o_v), h_nb, h_par, outlierTH_per_point, &F->work)) return r;
  }
  F->have_first = true;
  *sparsity_factor = sf;
  if (n_points) for (int l = 0; l < L; l++) n_points[l] = n[l];
  return 0;
}

int dmvio_hip_init_first_get_level(dmvio_hip_init_first* F, int lvl, float* u, float* v, float* my_type, int* neighbours10, int* parent) {
  if (!F) return failmsg("init_first_get_level: null init_first handle");
  std::lock_guard<std::mutex> lk(F->ctx->mu);
  if (!F->have_first) return failmsg("init_first_get_level: no point lists (the last dmvio_hip_initializer_set_first was refused or failed, or none has run)");
  if (lvl < 0 || lvl >= F->levels) return failmsg("init_first_get_level: level out of range");
  const FirstLevel& V = F->lv[lvl];
  const size_t n = (size_t)V.n;
  if (u) memcpy(u, V.pts.host<float>(V.o_u), sizeof(float) * n);
  if (v) memcpy(v, V.pts.host<float>(V.o_v), sizeof(float) * n);
  if (my_type) memcpy(my_type, V.pts.host<float>(V.o_type), sizeof(float) * n);
  if (neighbours10) memcpy(neighbours10, V.pts.host<int>(V.o_nb), sizeof(int) * 10 * n);
  if (parent) memcpy(parent, V.pts.host<int>(V.o_parent), sizeof(int) * n);
  return V.n;
}

int dmvio_hip_init_first_last_work(dmvio_hip_init_first* F, int* launches, int* uploads, int* downloads, int* waits) {
  if (!F) return failmsg("init_first_last_work: null init_first handle");
  std::lock_guard<std::mutex> lk(F->ctx->mu);
  F->work.report(launches, uploads, downloads, waits);
  return 0;
}

}  // extern "C"
