// C ABI of the pixel selector (include/dmvio_hip.h): PixelSelector::makeMaps on a resident frame, and the list FullSystem::makeNewTraces builds its points from.
#include <vector>
#include <cmath>
#include <cstring>
#include <algorithm>
#include "../../include/dmvio_hip.h"
#include "internal.h"
#include "select_kernels.hpp"
#include "select_batch_kernels.hpp"

using namespace dmv;

struct dmvio_hip_pixel_selector {
  dmvio_hip_ctx* ctx = nullptr;
  int w = 0, h = 0, nbW = 0, nbH = 0;
  int currentPotential = 3;   // PixelSelector2.cpp:49
  dmvio_hip_pixel_selector_settings S{};
  int ncell_max = 0;
  // device memory, all sized at creation for potential 1
  unsigned char* d_pattern = nullptr;   // randomPattern[w*h]
  float* d_lut = nullptr;               // 256
  float* d_ag = nullptr;                // absSquaredGrad [level 0 | level 1 | level 2]
  float *d_ths = nullptr, *d_thsS = nullptr;
  char* d_zero = nullptr;               // cleared before every select pass: [counters | mask | key2 | key3 | key4 | map]
  size_t zero_cap = 0;
  int* d_n2ex = nullptr;
  int2* d_tiles = nullptr;
  int* d_rn = nullptr;
  int *d_lu = nullptr, *d_lv = nullptr, *d_lt = nullptr;
  float *d_wu = nullptr, *d_wv = nullptr;
  int* h_counts = nullptr;              // pinned, SELC_COUNT ints
  // layout of d_zero of the last pass
  int* d_counters = nullptr;
  unsigned char* d_map = nullptr;
  // results of the last call
  int last_slot = -1, n_selected = 0, n_window = 0;
  int last_counts[3] = {0, 0, 0};
  std::vector<int> pass_pot, pass_counts;
  long long exact_runs = 0;
  std::vector<void*> allocs;
};

template <class T>
static int salloc(dmvio_hip_pixel_selector* s, T** p, size_t n) {
  HIPCHK(hipMalloc((void**)p, sizeof(T) * std::max<size_t>(n, 1)));
  HIPCHK(hipMemset(*p, 0, sizeof(T) * std::max<size_t>(n, 1)));
  HIPCHK(hipStreamSynchronize(nullptr));   // as ialloc() of capi_immature.hip
  s->allocs.push_back(*p);
  return 0;
}
#define SEL_READY(s) do { if (!(s)) return failmsg("null pixel selector handle"); HIPCHK(hipSetDevice((s)->ctx->device)); } while (0)

// geometry and scratch layout of one select() pass at potential `pot`: what the single call and a window of a batch share.  Sets s->d_counters / s->d_map.
struct SelLayout {
  SelGeom G;
  unsigned int* d_mask;
  unsigned long long *d_key2, *d_key3, *d_key4;
  size_t bytes;   // of d_zero, cleared before the pass
};
static int selectLayout(dmvio_hip_pixel_selector* s, int pot, float thFactor, SelLayout& L) {
  dmvio_hip_ctx* c = s->ctx;
  const int w = s->w, h = s->h, wh = w * h;
  SelGeom& G = L.G;
  G.w = w; G.h = h; G.w1 = c->wl[1]; G.w2 = c->wl[2];
  G.pot = std::min(pot, std::max(w, h));
  G.nb4x = (w + 4 * G.pot - 1) / (4 * G.pot);
  const int nb4y = (h + 4 * G.pot - 1) / (4 * G.pot);
  G.ncell = 16 * G.nb4x * nb4y;
  G.nbW = s->nbW;
  G.thFactor = thFactor;
  G.dw1 = s->S.gradDownweightPerLevel;
  G.dw2 = G.dw1 * G.dw1;   // :350-351
  G.useDir = s->S.selectDirectionDistribution != 0;
  if (G.ncell > s->ncell_max) return failmsg("pixel_selector: internal: cell count exceeds the scratch");
  const size_t N = G.ncell;
  size_t off = 0;
  s->d_counters = reinterpret_cast<int*>(s->d_zero + off); off += dmvPad(sizeof(int) * SELC_COUNT);
  L.d_mask = reinterpret_cast<unsigned int*>(s->d_zero + off); off += dmvPad(sizeof(unsigned int) * N);
  // the three key arrays lie back to back: k_sel_pick addresses them as one (N is a multiple of 16)
  L.d_key2 = reinterpret_cast<unsigned long long*>(s->d_zero + off); off += dmvPad(sizeof(unsigned long long) * (N + N / 4 + N / 16));
  L.d_key3 = L.d_key2 + N; L.d_key4 = L.d_key3 + N / 4;
  s->d_map = reinterpret_cast<unsigned char*>(s->d_zero + off); off += dmvPad((size_t)wh);
  if (off > s->zero_cap) return failmsg("pixel_selector: internal: scratch layout exceeds its allocation");
  L.bytes = off;
  return 0;
}

// one select() pass (PixelSelector2.cpp:311-454) at potential `pot` on the stream; the counters are copied into h_counts and waited for
static int selectPass(dmvio_hip_pixel_selector* s, int slot, int pot, float thFactor) {
  dmvio_hip_ctx* c = s->ctx;
  const int w = s->w, h = s->h, wh = w * h;
  SelLayout L;
  if (int r = selectLayout(s, pot, thFactor, L)) return r;
  const SelGeom& G = L.G;
  unsigned int* d_mask = L.d_mask;
  unsigned long long *d_key2 = L.d_key2, *d_key3 = L.d_key3, *d_key4 = L.d_key4;
  hipStream_t st = c->stream;
  HIPCHK(hipMemsetAsync(s->d_zero, 0, L.bytes, st));
  const float* I0 = c->frames.levelPtr(slot, 0);
  const float *ag0 = s->d_ag, *ag1 = ag0 + wh, *ag2 = ag1 + c->wl[1] * c->hl[1];
  hipLaunchKernelGGL(k_sel_cellmask, dim3((wh + 255) / 256), dim3(256), 0, st, I0, ag0, (const float*)s->d_thsS, G, d_mask);
  SelScanArgs A;
  A.n = G.ncell; A.charTH = 255; A.w = w; A.h = h;
  const int ntiles = (G.ncell + SEL_TILE - 1) / SEL_TILE;
  hipLaunchKernelGGL(k_sel_scanA<SEL_MODE_CELL>, dim3(ntiles), dim3(256), 0, st, A, (const unsigned int*)d_mask, (const unsigned char*)nullptr, (const int*)nullptr,
                     (const unsigned char*)nullptr, s->d_tiles);
  hipLaunchKernelGGL(k_sel_scanB, dim3(1), dim3(256), 0, st, s->d_tiles, ntiles, s->d_counters, (int)SELC_N2, (int)SELC_MIXED);
  hipLaunchKernelGGL(k_sel_scanC<SEL_MODE_CELL>, dim3(ntiles), dim3(256), 0, st, A, (const unsigned int*)d_mask, (unsigned char*)nullptr, (const int*)nullptr,
                     (const unsigned char*)nullptr, (const int2*)s->d_tiles, s->d_n2ex, (int*)nullptr, (int*)nullptr, (int*)nullptr, (float*)nullptr, (float*)nullptr);
  hipLaunchKernelGGL(k_sel_scan_exact, dim3(1), dim3(64), 0, st, (const unsigned int*)d_mask, G.ncell, (const unsigned char*)s->d_pattern, wh, s->d_n2ex, s->d_counters);
  hipLaunchKernelGGL(k_sel_pick, dim3((wh + 255) / 256), dim3(256), 0, st, I0, ag0, ag1, ag2, (const float*)s->d_thsS, (const unsigned char*)s->d_pattern,
                     (const int*)s->d_n2ex, G, d_key2);
  hipLaunchKernelGGL(k_sel_write, dim3((G.ncell + 1023) / 1024), dim3(1024), 0, st, (const int*)s->d_n2ex, (const unsigned long long*)d_key2, (const unsigned long long*)d_key3,
                     (const unsigned long long*)d_key4, G, s->d_map, s->d_counters);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s->h_counts, s->d_counters, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// The decision step of makeMaps' recursion (:203-245) after one select pass with counters n[]: records the pass, and either moves currentPotential and asks for another
// pass (true) or ends the recursion (false).  The single call and every window of a batched call run this one function.
struct SelRecursion {
  float numWant = 0, quotia = 0;
  int idealPotential = 0, recursionsLeft = 0;
};
static bool selectDecide(dmvio_hip_pixel_selector* s, const int* n, SelRecursion& R) {
  s->pass_pot.push_back(s->currentPotential);
  for (int k = 0; k < 3; k++) { s->pass_counts.push_back(n[k]); s->last_counts[k] = n[k]; }
  if (n[SELC_EXACT]) s->exact_runs++;
  const float numHave = (float)(n[0] + n[1] + n[2]);
  R.quotia = R.numWant / numHave;
  const float K = numHave * (s->currentPotential + 1) * (s->currentPotential + 1);
  R.idealPotential = (int)(sqrtf(K / R.numWant) - 1);   // round down
  if (R.idealPotential < 1) R.idealPotential = 1;
  if (R.recursionsLeft > 0 && (double)R.quotia > 1.25 && s->currentPotential > 1) {
    if (R.idealPotential >= s->currentPotential) R.idealPotential = s->currentPotential - 1;
    s->currentPotential = R.idealPotential;
    R.recursionsLeft--;
    return true;
  }
  if (R.recursionsLeft > 0 && (double)R.quotia < 0.25) {
    if (R.idealPotential <= s->currentPotential) R.idealPotential = s->currentPotential + 1;
    s->currentPotential = R.idealPotential;
    R.recursionsLeft--;
    return true;
  }
  return false;
}

extern "C" {

void dmvio_hip_pixel_selector_default_settings(dmvio_hip_pixel_selector_settings* s) {
  if (!s) return;
  s->minGradHistCut = 0.5f;               // settings.cpp:167
  s->minGradHistAdd = 7.0f;               // settings.cpp:168
  s->gradDownweightPerLevel = 0.75f;      // settings.cpp:169
  s->selectDirectionDistribution = 1;     // settings.cpp:170
}

dmvio_hip_pixel_selector* dmvio_hip_pixel_selector_create(dmvio_hip_ctx* ctx, const unsigned char* random_pattern_wh) {
  if (!ctx) { failmsg("pixel_selector_create: null context"); return nullptr; }
  if (!random_pattern_wh) { failmsg("pixel_selector_create: random_pattern_wh is NULL (the caller supplies PixelSelector's randomPattern, w*h bytes)"); return nullptr; }
  if (ctx->w % 16 != 0 || ctx->h % 16 != 0) { failmsg("pixel_selector_create: height or width not divisible by 16 (PixelSelector2.cpp:53-61)"); return nullptr; }
  if (ctx->levels < 3) { failmsg("pixel_selector_create: the selector reads pyramid levels 0..2"); return nullptr; }
  HIPCHKP(hipSetDevice(ctx->device));
  dmvio_hip_pixel_selector* s = new dmvio_hip_pixel_selector();
  s->ctx = ctx; s->w = ctx->w; s->h = ctx->h; s->nbW = ctx->w / 16; s->nbH = ctx->h / 16;
  dmvio_hip_pixel_selector_default_settings(&s->S);
  const size_t wh = (size_t)s->w * s->h;
  s->ncell_max = 16 * ((s->w + 3) / 4) * ((s->h + 3) / 4);
  const size_t N = s->ncell_max;
  s->zero_cap = dmvPad(sizeof(int) * SELC_COUNT) + dmvPad(4 * N) + dmvPad(8 * N) + dmvPad(8 * (N / 4)) + dmvPad(8 * (N / 16)) + dmvPad(wh);
  const size_t nag = wh + (size_t)ctx->wl[1] * ctx->hl[1] + (size_t)ctx->wl[2] * ctx->hl[2];
  const size_t ntiles = (std::max(N, wh) + SEL_TILE - 1) / SEL_TILE + 1;
  if (salloc(s, &s->d_pattern, wh) || salloc(s, &s->d_lut, 256) || salloc(s, &s->d_ag, nag) || salloc(s, &s->d_ths, (size_t)s->nbW * s->nbH) ||
      salloc(s, &s->d_thsS, (size_t)s->nbW * s->nbH) || salloc(s, &s->d_zero, s->zero_cap) || salloc(s, &s->d_n2ex, N + 1) || salloc(s, &s->d_tiles, ntiles) ||
      salloc(s, &s->d_rn, wh) || salloc(s, &s->d_lu, wh) || salloc(s, &s->d_lv, wh) || salloc(s, &s->d_lt, wh) || salloc(s, &s->d_wu, wh) || salloc(s, &s->d_wv, wh) ||
      hipHostMalloc((void**)&s->h_counts, sizeof(int) * SELC_COUNT, hipHostMallocDefault) != hipSuccess ||
      hipMemcpy(s->d_pattern, random_pattern_wh, wh, hipMemcpyHostToDevice) != hipSuccess) {
    if (dmv_err().empty()) failmsg("pixel_selector_create: allocation failed");
    for (void* p : s->allocs) hipFree(p);
    if (s->h_counts) hipHostFree(s->h_counts);
    delete s;
    return nullptr;
  }
  s->d_counters = reinterpret_cast<int*>(s->d_zero);
  s->d_map = reinterpret_cast<unsigned char*>(s->d_zero);
  return s;
}
void dmvio_hip_pixel_selector_destroy(dmvio_hip_pixel_selector* s) {
  if (!s) return;
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  for (void* p : s->allocs) hipFree(p);
  if (s->h_counts) hipHostFree(s->h_counts);
  delete s;
}
int dmvio_hip_pixel_selector_set_settings(dmvio_hip_pixel_selector* s, const dmvio_hip_pixel_selector_settings* st) {
  if (!s || !st) return failmsg("pixel_selector_set_settings: null argument");
  s->S = *st;
  return 0;
}
int dmvio_hip_pixel_selector_get_potential(dmvio_hip_pixel_selector* s) { return s ? s->currentPotential : failmsg("pixel_selector_get_potential: null handle"); }
int dmvio_hip_pixel_selector_set_potential(dmvio_hip_pixel_selector* s, int potential) {
  if (!s || potential < 1) return failmsg("pixel_selector_set_potential: bad argument");
  s->currentPotential = potential;
  return 0;
}

int dmvio_hip_pixel_selector_make_maps(dmvio_hip_pixel_selector* s, int slot, const float* B_lut256, float density, int recursions_left, float th_factor, int* n_selected,
                                       int counts3[3], float* map_out_host) {
  SEL_READY(s);
  std::lock_guard<std::mutex> lk(s->ctx->mu);
  return dmv_selector_make_maps_locked(s, slot, B_lut256, density, recursions_left, th_factor, n_selected, counts3, map_out_host);
}
}  // extern "C"

// makeMaps under the context's lock, which the caller holds (the entry point above; dmvio_hip_initializer_set_first in capi_init_first.hip)
int dmv_selector_make_maps_locked(dmvio_hip_pixel_selector* s, int slot, const float* B_lut256, float density, int recursions_left, float th_factor, int* n_selected,
                                  int counts3[3], float* map_out_host) {
  dmvio_hip_ctx* c = s->ctx;
  if (slot < 0 || slot >= c->n_slots) return failmsg("pixel_selector_make_maps: frame slot out of range");
  if (!n_selected) return failmsg("pixel_selector_make_maps: n_selected is NULL");
  if (int r = dmv_ensure_row_major_locked(c, slot)) return r;
  hipStream_t st = c->stream;
  const int w = s->w, h = s->h, wh = w * h;
  // FrameHessian::makeImages' absSquaredGrad and makeHists (the reference keeps the histogram per FrameHessian pointer, :200: same values)
  if (B_lut256) HIPCHK(c->bounce.h2d(s->d_lut, B_lut256, sizeof(float) * 256, st));
  const int nag = wh + c->wl[1] * c->hl[1] + c->wl[2] * c->hl[2];
  hipLaunchKernelGGL(k_sel_absgrad, dim3((nag + 255) / 256), dim3(256), 0, st, c->frames.levelPtr(slot, 0), c->frames.levelPtr(slot, 1), c->frames.levelPtr(slot, 2), w, h, c->wl[1], c->hl[1],
                     c->wl[2], c->hl[2], (const float*)(B_lut256 ? s->d_lut : nullptr), s->d_ag);
  hipLaunchKernelGGL(k_sel_hist, dim3(s->nbW * s->nbH), dim3(256), 0, st, (const float*)s->d_ag, w, h, s->nbW, s->S.minGradHistCut, s->S.minGradHistAdd, s->d_ths);
  hipLaunchKernelGGL(k_sel_smooth, dim3((s->nbW * s->nbH + 255) / 256), dim3(256), 0, st, (const float*)s->d_ths, s->nbW, s->nbH, s->d_thsS);
  HIPCHK(hipGetLastError());

  // makeMaps (:158-273); its recursion is this loop
  s->pass_pot.clear(); s->pass_counts.clear();
  SelRecursion R;
  R.numWant = density; R.idealPotential = s->currentPotential; R.recursionsLeft = recursions_left;
  for (;;) {
    if (int r = selectPass(s, slot, s->currentPotential, th_factor)) return r;
    if (!selectDecide(s, s->h_counts, R)) break;
  }
  const float quotia = R.quotia;
  const int idealPotential = R.idealPotential;
  // sub-selection (:247-265), compaction in raster order, the makeNewTraces window
  SelScanArgs A;
  A.n = wh; A.w = w; A.h = h; A.charTH = 255;
  const int ntiles = (wh + SEL_TILE - 1) / SEL_TILE;
  const int* rn = nullptr;
  if ((double)quotia < 0.95) {
    A.charTH = (int)(unsigned char)(255 * quotia);
    hipLaunchKernelGGL(k_sel_scanA<SEL_MODE_NZ>, dim3(ntiles), dim3(256), 0, st, A, (const unsigned int*)nullptr, (const unsigned char*)s->d_map, (const int*)nullptr,
                       (const unsigned char*)nullptr, s->d_tiles);
    hipLaunchKernelGGL(k_sel_scanB, dim3(1), dim3(256), 0, st, s->d_tiles, ntiles, s->d_counters, (int)SELC_NZ, -1);
    hipLaunchKernelGGL(k_sel_scanC<SEL_MODE_NZ>, dim3(ntiles), dim3(256), 0, st, A, (const unsigned int*)nullptr, s->d_map, (const int*)nullptr, (const unsigned char*)nullptr,
                       (const int2*)s->d_tiles, s->d_rn, (int*)nullptr, (int*)nullptr, (int*)nullptr, (float*)nullptr, (float*)nullptr);
    rn = s->d_rn;
  }
  hipLaunchKernelGGL(k_sel_scanA<SEL_MODE_SURV>, dim3(ntiles), dim3(256), 0, st, A, (const unsigned int*)nullptr, (const unsigned char*)s->d_map, rn,
                     (const unsigned char*)s->d_pattern, s->d_tiles);
  hipLaunchKernelGGL(k_sel_scanB, dim3(1), dim3(256), 0, st, s->d_tiles, ntiles, s->d_counters, (int)SELC_NSEL, (int)SELC_NWIN);
  hipLaunchKernelGGL(k_sel_scanC<SEL_MODE_SURV>, dim3(ntiles), dim3(256), 0, st, A, (const unsigned int*)nullptr, s->d_map, rn, (const unsigned char*)s->d_pattern,
                     (const int2*)s->d_tiles, (int*)nullptr, s->d_lu, s->d_lv, s->d_lt, s->d_wu, s->d_wv);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s->h_counts, s->d_counters, sizeof(int) * 8, hipMemcpyDeviceToHost, st));
  size_t moff = 0;
  if (map_out_host) {
    HIPCHK(c->bounce.reserve((size_t)wh, st, &moff));
    HIPCHK(hipMemcpyAsync(c->bounce.h + moff, s->d_map, (size_t)wh, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c->bounce.finish(st));
  if (map_out_host) {
    const unsigned char* m = reinterpret_cast<const unsigned char*>(c->bounce.h + moff);
    for (int i = 0; i < wh; i++) map_out_host[i] = (float)m[i];
  }
  s->currentPotential = idealPotential;   // :273
  s->n_selected = s->h_counts[SELC_NSEL];
  s->n_window = s->h_counts[SELC_NWIN];
  s->last_slot = slot;
  *n_selected = s->n_selected;
  if (counts3) for (int k = 0; k < 3; k++) counts3[k] = s->last_counts[k];
  return 0;
}

extern "C" {

int dmvio_hip_pixel_selector_get_selection(dmvio_hip_pixel_selector* s, int* u, int* v, int* type) {
  SEL_READY(s);
  dmvio_hip_ctx* c = s->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  if (s->last_slot < 0) return failmsg("pixel_selector_get_selection: no make_maps call yet");
  const size_t n = s->n_selected;
  if (u) HIPCHK(c->bounce.d2h(u, s->d_lu, sizeof(int) * n, c->stream));
  if (v) HIPCHK(c->bounce.d2h(v, s->d_lv, sizeof(int) * n, c->stream));
  if (type) HIPCHK(c->bounce.d2h(type, s->d_lt, sizeof(int) * n, c->stream));
  HIPCHK(c->bounce.finish(c->stream));
  return s->n_selected;
}
int dmvio_hip_pixel_selector_get_thresholds(dmvio_hip_pixel_selector* s, float* ths, float* thsSmoothed) {
  SEL_READY(s);
  dmvio_hip_ctx* c = s->ctx;
  std::lock_guard<std::mutex> lk(c->mu);
  const size_t n = (size_t)s->nbW * s->nbH;
  if (ths) HIPCHK(c->bounce.d2h(ths, s->d_ths, sizeof(float) * n, c->stream));
  if (thsSmoothed) HIPCHK(c->bounce.d2h(thsSmoothed, s->d_thsS, sizeof(float) * n, c->stream));
  HIPCHK(c->bounce.finish(c->stream));
  return 0;
}
int dmvio_hip_pixel_selector_get_passes(dmvio_hip_pixel_selector* s, int max_passes, int* potential, int* counts3) {
  if (!s) return failmsg("pixel_selector_get_passes: null handle");
  const int n = (int)s->pass_pot.size();
  for (int i = 0; i < n && i < max_passes; i++) {
    if (potential) potential[i] = s->pass_pot[i];
    if (counts3) for (int k = 0; k < 3; k++) counts3[3 * i + k] = s->pass_counts[3 * i + k];
  }
  return n;
}
int dmvio_hip_pixel_selector_get_stats(dmvio_hip_pixel_selector* s, long long stats4[4]) {
  if (!s || !stats4) return failmsg("pixel_selector_get_stats: null argument");
  stats4[0] = s->exact_runs; stats4[1] = (long long)s->pass_pot.size(); stats4[2] = s->n_selected; stats4[3] = s->n_window;
  return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------------ W keyframes per call
// makeMaps for W selectors of one context.  The recursion stays on the host, in rounds: round r runs one select pass for every window that is still recursing, each at its
// own potential; the counters of all windows come back in one copy behind one stream wait, and selectDecide() moves every window on.  The final phase (sub-selection,
// raster compaction, makeNewTraces list) runs once for all windows.  Every round writes one pinned slab [SelWin x W | B tables] and uploads it in one copy; the slab is
// rewritten only after the wait that ends the round before.
struct dmvio_hip_pixel_selector_batch {
  dmvio_hip_ctx* ctx = nullptr;
  int max_windows = 0;
  DmvSlab slab;                                   // max_windows x (SelWin | 256 floats), sized at creation (dmvSelSlabBytes, batch_slab.hpp)
  DmvSlab counts;                                 // max_windows x SELC_COUNT ints
  char* d_traces = nullptr;                       // max_windows records of dmvio_hip_immature_add_selected_batch (capi_immature.hip)
  size_t traces_bytes = 0;
};
enum { SEL_TRACES_RECORD = 512 };   // bytes reserved per window in d_traces (capi_immature.hip checks its record against it)

// the record of window `k` for a select pass at its selector's current potential (active) or for a phase it only watches (inactive: the layout of its last pass stays)
static int selRecord(dmvio_hip_pixel_selector_batch* b, SelWin& R, size_t lut_off, int k, const dmvio_hip_pixel_selector_window& V, bool pass) {
  dmvio_hip_pixel_selector* s = V.sel;
  dmvio_hip_ctx* c = b->ctx;
  memset(&R, 0, sizeof(R));
  R.I0 = c->frames.levelPtr(V.slot, 0); R.I1 = c->frames.levelPtr(V.slot, 1); R.I2 = c->frames.levelPtr(V.slot, 2);
  if (V.B_lut256) {
    const auto B = b->slab.put<float>(lut_off);
    memcpy(B.h + 256 * (size_t)k, V.B_lut256, sizeof(float) * 256);
    R.B = B.d + 256 * (size_t)k;
  }
  R.ag = s->d_ag; R.ths = s->d_ths; R.thsS = s->d_thsS; R.pattern = s->d_pattern;
  R.counters = b->counts.dev<int>(0) + (size_t)k * SELC_COUNT;
  R.n2ex = s->d_n2ex; R.tiles = s->d_tiles; R.rn = s->d_rn; R.lu = s->d_lu; R.lv = s->d_lv; R.lt = s->d_lt; R.wu = s->d_wu; R.wv = s->d_wv;
  R.h1 = c->hl[1]; R.h2 = c->hl[2]; R.nbH = s->nbH;
  R.histCut = s->S.minGradHistCut; R.histAdd = s->S.minGradHistAdd;
  R.G.w = s->w; R.G.h = s->h; R.G.w1 = c->wl[1]; R.G.w2 = c->wl[2]; R.G.nbW = s->nbW;
  R.A.w = s->w; R.A.h = s->h; R.A.charTH = 255;
  if (pass) {
    SelLayout L;
    if (int r = selectLayout(s, s->currentPotential, V.th_factor, L)) return r;
    R.G = L.G;
    R.zero = reinterpret_cast<uint4*>(s->d_zero); R.zero_words = (int)(L.bytes / 16);
    R.mask = L.d_mask; R.keys = L.d_key2;
    R.A.n = L.G.ncell;
    R.active = 1;
  }
  R.map = s->d_map;
  return 0;
}

extern "C" {

dmvio_hip_pixel_selector_batch* dmvio_hip_pixel_selector_batch_create(dmvio_hip_ctx* ctx, int max_windows) {
  if (!ctx) { failmsg("pixel_selector_batch_create: null context"); return nullptr; }
  if (max_windows < 1 || max_windows > 65535) { failmsg("pixel_selector_batch_create: max_windows out of range (1..65535)"); return nullptr; }
  HIPCHKP(hipSetDevice(ctx->device));
  dmvio_hip_pixel_selector_batch* b = new dmvio_hip_pixel_selector_batch();
  b->ctx = ctx; b->max_windows = max_windows;
  b->traces_bytes = (size_t)SEL_TRACES_RECORD * max_windows;
  if (b->slab.create(dmvSelSlabBytes(sizeof(SelWin), max_windows)) || b->counts.create(sizeof(int) * SELC_COUNT * (size_t)max_windows) ||
      hipMalloc((void**)&b->d_traces, b->traces_bytes) != hipSuccess) {
    failmsg("pixel_selector_batch_create: allocation failed");
    b->slab.release(); b->counts.release();
    delete b;
    return nullptr;
  }
  return b;
}
void dmvio_hip_pixel_selector_batch_destroy(dmvio_hip_pixel_selector_batch* b) {
  if (!b) return;
  hipSetDevice(b->ctx->device);
  hipStreamSynchronize(b->ctx->stream);
  b->slab.release(); b->counts.release(); hipFree(b->d_traces);
  delete b;
}

int dmvio_hip_pixel_selector_make_maps_batch(dmvio_hip_pixel_selector_batch* b, int W, dmvio_hip_pixel_selector_window* win) {
  if (int r = dmvBatchHead(b, W, b ? b->max_windows : 0, win, "pixel_selector_make_maps_batch")) return r;
  if (W == 0) return 0;
  dmvio_hip_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  // every refusal before anything is enqueued or any handle touched
  const int rep = dmvFirstRepeated(win, W, &dmvio_hip_pixel_selector_window::sel);
  for (int k = 0; k < W; k++) {
    const dmvio_hip_pixel_selector_window& V = win[k];
    if (!V.sel) return failmsg("pixel_selector_make_maps_batch: a selector handle is NULL");
    if (V.sel->ctx != c) return failmsg("pixel_selector_make_maps_batch: a selector belongs to another context");
    if (k == rep) return failmsg("pixel_selector_make_maps_batch: a selector appears twice");
    if (V.slot < 0 || V.slot >= c->n_slots) return failmsg("pixel_selector_make_maps_batch: frame slot out of range");
  }
  for (int k = 0; k < W; k++) if (int r = dmv_ensure_row_major_locked(c, win[k].slot)) return r;
  hipStream_t st = c->stream;
  const int w = c->w, h = c->h, wh = w * h;
  DmvCursor L;
  dmvRecords(L, sizeof(SelWin), W);
  const size_t lut_off = dmvSelLuts(L, W), cnt_bytes = sizeof(int) * SELC_COUNT * (size_t)W;
  if (int r = b->slab.begin(st)) return r;   // (every round ends in a wait: the slab is free to rewrite)
  SelWin* R = b->slab.host<SelWin>(0);
  const SelWin* D = b->slab.dev<const SelWin>(0);
  const int* h_counts = b->counts.host<int>(0);
  std::vector<SelRecursion> rec(W);
  std::vector<char> running(W, 1);
  for (int k = 0; k < W; k++) {
    dmvio_hip_pixel_selector* s = win[k].sel;
    s->pass_pot.clear(); s->pass_counts.clear();
    rec[k].numWant = win[k].density; rec[k].idealPotential = s->currentPotential; rec[k].recursionsLeft = win[k].recursions_left;
  }
  // makeMaps (:158-273): its recursion is this loop, one round per pass of the window that recurses longest
  for (int round = 0;; round++) {
    int zmax = 0, tmax = 0, cmax = 0;
    for (int k = 0; k < W; k++) {
      if (int r = selRecord(b, R[k], lut_off, k, win[k], running[k] != 0)) return r;
      if (!running[k]) continue;
      zmax = std::max(zmax, R[k].zero_words); tmax = std::max(tmax, (R[k].A.n + SEL_TILE - 1) / SEL_TILE); cmax = std::max(cmax, R[k].G.ncell);
    }
    if (int r = b->slab.upload(st, L.bytes())) return r;
    if (round == 0) {
      // FrameHessian::makeImages' absSquaredGrad and makeHists of every window
      const int nag = wh + c->wl[1] * c->hl[1] + c->wl[2] * c->hl[2];
      const int nb = (w / 16) * (h / 16);
      hipLaunchKernelGGL(k_sel_absgrad_b, dim3((nag + 255) / 256, W), dim3(256), 0, st, D);
      hipLaunchKernelGGL(k_sel_hist_b, dim3(nb, W), dim3(256), 0, st, D);
      hipLaunchKernelGGL(k_sel_smooth_b, dim3((nb + 255) / 256, W), dim3(256), 0, st, D);
    }
    // the scratch clear of all active windows is one fill
    hipLaunchKernelGGL(k_sel_clear_b, dim3((zmax + 255) / 256, W), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_sel_cellmask_b, dim3((wh + 255) / 256, W), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_sel_scanA_b<SEL_MODE_CELL>, dim3(tmax, W), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_sel_scanB_b, dim3(W), dim3(256), 0, st, D, (int)SEL_MODE_CELL, (int)SELC_N2, (int)SELC_MIXED);
    hipLaunchKernelGGL(k_sel_scanC_b<SEL_MODE_CELL>, dim3(tmax, W), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_sel_scan_exact_b, dim3(W), dim3(64), 0, st, D);
    hipLaunchKernelGGL(k_sel_pick_b, dim3((wh + 255) / 256, W), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_sel_write_b, dim3((cmax + 1023) / 1024, W), dim3(1024), 0, st, D);
    HIPCHK(hipGetLastError());
    if (int r = b->counts.download(st, 0, cnt_bytes)) return r;
    if (int r = b->slab.wait(st)) return r;   // the one wait of the round
    bool any = false;
    for (int k = 0; k < W; k++) {
      if (!running[k]) continue;
      running[k] = selectDecide(win[k].sel, h_counts + (size_t)k * SELC_COUNT, rec[k]) ? 1 : 0;
      any = any || running[k];
    }
    if (!any) break;
  }
  // sub-selection (:247-265) for the windows with quotia < 0.95, compaction in raster order, the makeNewTraces window: once for all windows
  bool anySub = false;
  int nmaps = 0;
  for (int k = 0; k < W; k++) {
    if (int r = selRecord(b, R[k], lut_off, k, win[k], false)) return r;
    R[k].A.n = wh;
    if ((double)rec[k].quotia < 0.95) {
      R[k].A.charTH = (int)(unsigned char)(255 * rec[k].quotia);
      R[k].sub = 1;
      anySub = true;
    }
    if (win[k].map_out_host) nmaps++;
  }
  if (int r = b->slab.upload(st, L.bytes())) return r;
  const int ntiles = (wh + SEL_TILE - 1) / SEL_TILE;
  if (anySub) {
    hipLaunchKernelGGL(k_sel_scanA_b<SEL_MODE_NZ>, dim3(ntiles, W), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_sel_scanB_b, dim3(W), dim3(256), 0, st, D, (int)SEL_MODE_NZ, (int)SELC_NZ, -1);
    hipLaunchKernelGGL(k_sel_scanC_b<SEL_MODE_NZ>, dim3(ntiles, W), dim3(256), 0, st, D);
  }
  hipLaunchKernelGGL(k_sel_scanA_b<SEL_MODE_SURV>, dim3(ntiles, W), dim3(256), 0, st, D);
  hipLaunchKernelGGL(k_sel_scanB_b, dim3(W), dim3(256), 0, st, D, (int)SEL_MODE_SURV, (int)SELC_NSEL, (int)SELC_NWIN);
  hipLaunchKernelGGL(k_sel_scanC_b<SEL_MODE_SURV>, dim3(ntiles, W), dim3(256), 0, st, D);
  HIPCHK(hipGetLastError());
  if (int r = b->counts.download(st, 0, cnt_bytes)) return r;
  // the status maps the caller asked for come back through the bounce buffer: ONE reservation (a second one could drain and rewind the staging area under the first)
  size_t moff = 0;
  const size_t mstep = dmvPad((size_t)wh);
  if (nmaps) {
    HIPCHK(c->bounce.reserve(mstep * nmaps, st, &moff));
    int j = 0;
    for (int k = 0; k < W; k++)
      if (win[k].map_out_host) HIPCHK(hipMemcpyAsync(c->bounce.h + moff + mstep * (j++), win[k].sel->d_map, (size_t)wh, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c->bounce.finish(st));   // the one wait of the final phase
  b->slab.settled();
  int j = 0;
  for (int k = 0; k < W; k++) {
    dmvio_hip_pixel_selector* s = win[k].sel;
    if (win[k].map_out_host) {
      const unsigned char* m = reinterpret_cast<const unsigned char*>(c->bounce.h + moff + mstep * (j++));
      for (int i = 0; i < wh; i++) win[k].map_out_host[i] = (float)m[i];
    }
    const int* hc = h_counts + (size_t)k * SELC_COUNT;
    s->currentPotential = rec[k].idealPotential;   // :273
    s->n_selected = hc[SELC_NSEL];
    s->n_window = hc[SELC_NWIN];
    s->last_slot = win[k].slot;
    win[k].n_selected = s->n_selected;
    for (int q = 0; q < 3; q++) win[k].counts3[q] = s->last_counts[q];
  }
  return 0;
}

}  // extern "C"

// the batch's context, size and record area for dmvio_hip_immature_add_selected_batch (capi_immature.hip): `bytes` per window must fit SEL_TRACES_RECORD
int dmv_selector_batch_traces(dmvio_hip_pixel_selector_batch* b, size_t record_bytes, dmvio_hip_ctx** ctx, int* max_windows, char** d_records) {
  if (!b) return failmsg("immature_add_selected_batch: null batch handle");
  if (record_bytes > (size_t)SEL_TRACES_RECORD) return failmsg("immature_add_selected_batch: internal: record larger than the batch reserves");
  *ctx = b->ctx; *max_windows = b->max_windows; *d_records = b->d_traces;
  return 0;
}
int dmv_selector_window_list(dmvio_hip_pixel_selector* s, dmvio_hip_ctx** ctx, const float** d_u, const float** d_v) {
  if (!s) return failmsg("null pixel selector handle");
  if (s->last_slot < 0) return failmsg("immature_add_selected: the selector has no selection yet (dmvio_hip_pixel_selector_make_maps)");
  *ctx = s->ctx; *d_u = s->d_wu; *d_v = s->d_wv;
  return s->n_window;
}
const unsigned char* dmv_selector_map(dmvio_hip_pixel_selector* s) { return s->d_map; }
dmvio_hip_ctx* dmv_selector_ctx(dmvio_hip_pixel_selector* s) { return s->ctx; }
