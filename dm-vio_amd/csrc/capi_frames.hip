// libdmvio_hip.so — C ABI implementation (include/dmvio_hip.h), library basics and the frame store: error string, context, streams, pyramid builds, undistorter,
// downloads, the result.txt writer.  gfx950 only.  The only unit that compiles image_kernels.hpp.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>
#include <algorithm>

#include "../../include/dmvio_hip.h"
#include "common.h"
#include "lie_dev.h"
#include "image_kernels.hpp"

using namespace dmv;

#include "internal.h"

std::string& dmv_err() { static thread_local std::string e; return e; }
unsigned int& dmv_err_epoch() { static thread_local unsigned int n = 0; return n; }

extern "C" {

const char* dmvio_hip_last_error(void) { return dmv_err().c_str(); }

int dmvio_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static int pyrLevels(int w, int h) {
  // setGlobalCalib (src/dso/util/globalCalib.cpp:47-55)
  int wl = w, hl = h, used = 1;
  while (wl % 2 == 0 && hl % 2 == 0 && wl * hl > 5000 && used < DMV_MAX_LEVELS) { wl /= 2; hl /= 2; used++; }
  return used;
}

// tile shape of the LDS-tile pyramid build: 2^tw_log2 pixels wide, PYR_TILE_PX / 2^tw_log2 high
static void setPyramidTile(dmvio_hip_ctx* c, int tw_log2) {
  c->pg.tw_log2 = tw_log2;
  const int TW = 1 << tw_log2, TH = PYR_TILE_PX >> tw_log2;
  c->pg.tiles_x = (c->w + TW - 1) / TW; c->pg.tiles_y = (c->h + TH - 1) / TH;
}

// geometry and device memory of a fresh context; on failure the caller destroys the partial handle
static int ctxInit(dmvio_hip_ctx* c) {
  const int w = c->w, h = c->h, n_frame_slots = c->n_slots;
  c->levels = pyrLevels(w, h);
  size_t off = 0;
  for (int l = 0; l < c->levels; l++) {
    c->wl[l] = w >> l; c->hl[l] = h >> l;
    c->fs_.level_off[l] = off;
    off += (size_t)c->wl[l] * c->hl[l];
  }
  c->fs_.levels = c->levels;
  c->fs_.slot_stride = (off + 63) & ~(size_t)63;
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIPCHK(hipMalloc((void**)&c->fs_.base, sizeof(float) * c->fs_.slot_stride * n_frame_slots));
  HIPCHK(hipMemsetAsync(c->fs_.base, 0, sizeof(float) * c->fs_.slot_stride * n_frame_slots, c->stream));
  HIPCHK(hipMalloc((void**)&c->fs_.build_gen, sizeof(unsigned int) * 3 * n_frame_slots));   // build_gen | bad_gen: equal (0) = not known to be clean | pend_gen: 0 = built
  HIPCHK(hipMemsetAsync(c->fs_.build_gen, 0, sizeof(unsigned int) * 3 * n_frame_slots, c->stream));
  c->fs_.bad_gen = c->fs_.build_gen + n_frame_slots;
  c->h_pending.assign(n_frame_slots, 0);
  c->slot_stamp.assign(n_frame_slots, 0u);
  HIPCHK(hipMalloc((void**)&c->fs_.lvl0, sizeof(const float*) * n_frame_slots));
  c->h_lvl0.resize(n_frame_slots);
  for (int s = 0; s < n_frame_slots; s++) c->h_lvl0[s] = c->fs_.own_level(s, 0);
  HIPCHK(hipMemcpyAsync(c->fs_.lvl0, c->h_lvl0.data(), sizeof(const float*) * n_frame_slots, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMalloc((void**)&c->fs_.tiled0, n_frame_slots));
  HIPCHK(hipMemsetAsync(c->fs_.tiled0, 0, n_frame_slots, c->stream));
  c->h_tiled.assign(n_frame_slots, 0);
  HIPCHK(hipMalloc((void**)&c->d_upload, sizeof(float) * w * h));
  c->pg.levels = c->levels;
  for (int l = 0; l < c->levels; l++) { c->pg.w[l] = c->wl[l]; c->pg.h[l] = c->hl[l]; }
  // tile shape of the pyramid build: as wide as the image (contiguous level-0 memory per workgroup), at least 2^(levels-1) rows for the 2x2 reductions
  int twl = 9;
  while (twl > 7 && ((1 << (twl - 1)) >= w || (PYR_TILE_PX >> twl) < (1 << (c->levels - 1)))) twl--;
  setPyramidTile(c, twl);
  HIPCHK(hipMalloc((void**)&c->d_f3, sizeof(float) * 3 * w * h));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

dmvio_hip_ctx* dmvio_hip_create(int device, int w, int h, int n_frame_slots) {
  if (w <= 0 || h <= 0 || n_frame_slots <= 0) { failmsg("dmvio_hip_create: bad arguments"); return nullptr; }
  int ndev = 0;
  HIPCHKP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) { failmsg("dmvio_hip_create: no such device"); return nullptr; }
  HIPCHKP(hipSetDevice(device));
  dmvio_hip_ctx* c = new dmvio_hip_ctx();
  c->device = device; c->w = w; c->h = h; c->n_slots = n_frame_slots;
  if (ctxInit(c)) { dmvio_hip_destroy(c); return nullptr; }   // releases what was allocated; the error text stays
  return c;
}

// Tile shape of the LDS-tile pyramid build (k_build_pyramids / k_build_pyramids_raw): 2^tw_log2 pixels wide, 4096 / 2^tw_log2 high; 7 .. 9, and the tile must keep
// 2^(levels-1) rows.  A measurement knob (profiles/r03_stream_ceilings.md); the default is as wide as the image allows.
int dmvio_hip_set_pyramid_tile_log2(dmvio_hip_ctx* c, int tw_log2) {
  if (!c) return failmsg("null context");
  if (tw_log2 < 7 || tw_log2 > 9 || (PYR_TILE_PX >> tw_log2) < (1 << (c->levels - 1))) return failmsg("set_pyramid_tile_log2: 7 .. 9, with at least 2^(levels-1) rows per tile");
  std::lock_guard<std::mutex> lk(c->mu);
  setPyramidTile(c, tw_log2);
  return 0;
}

void dmvio_hip_destroy(dmvio_hip_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  // (slots that still wait for a deferred build are not built: nothing can read them any more, and their images need not outlive the context)
  if (c->stream) hipStreamSynchronize(c->stream);   // (null only in a handle whose creation failed)
  hipFree(c->fs_.base);
  hipFree(c->fs_.build_gen);
  hipFree(c->fs_.lvl0);
  hipFree(c->fs_.tiled0);
  hipFree(c->d_upload);
  c->bounce.release();
  hipFree(c->d_f3);
  for (auto& L : c->slot_lists) { if (L.d) hipFree(L.d); if (L.h) hipHostFree(L.h); }
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
  delete c;
}

int dmvio_hip_pyr_levels(const dmvio_hip_ctx* c) { return c ? c->levels : 0; }

int dmvio_hip_set_stream(dmvio_hip_ctx* c, void* s) {
  if (!c) return failmsg("null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  if (int r = dmv_flush_pending(c, 0)) return r;   // a deferred attach is finished on the stream it was made on
  HIPCHK(hipStreamSynchronize(c->stream));
  if (s) {
    if (c->own_stream) { HIPCHK(hipStreamDestroy(c->stream)); }
    c->stream = (hipStream_t)s; c->own_stream = false;
  } else if (!c->own_stream) {
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true;
  }
  return 0;
}

static hipStream_t buildStream(const dmvio_hip_ctx* c) { return c->build_stream ? c->build_stream : c->stream; }
// The stream the BATCHED pyramid builds (dmvio_hip_frames_from_device_batch / _attach_device_batch / _from_raw_device_batch) are enqueued on; NULL (default): the context's
// stream.  With a stream of its own the build of batch k+1 overlaps the tracking of batch k — the build is bound by HBM, k_track_lm by its L1 miss path and VALU issue.  The
// CALLER orders the two streams (events): a build must not start before the consumers of the slots it rewrites have finished, a consumer not before the build of its slots.
int dmvio_hip_set_build_stream(dmvio_hip_ctx* c, void* s) {
  if (!c) return failmsg("null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  if (int r = dmv_flush_pending(c, 0)) return r;   // with a build stream nothing is deferred: what waits is built now, on the context's stream
  HIPCHK(hipStreamSynchronize(buildStream(c)));
  c->build_stream = (hipStream_t)s;
  return 0;
}

int dmvio_hip_synchronize(dmvio_hip_ctx* c) {
  if (!c) return failmsg("null ctx");
  HIPCHK(hipSetDevice(c->device));
  if (int r = dmv_flush_pending(c, 0)) return r;   // after a synchronize every slot is built: the caller may read the store from any stream
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->build_stream) HIPCHK(hipStreamSynchronize(c->build_stream));
  return 0;
}

// ------------------------------------------------------------------ frames
// the wave-autonomous builds (a 4 x 8 pixel block per thread, levels in registers: image_kernels.hpp) take pyramids of at most four levels on images whose sides are
// multiples of 8; everything else (and dmvio_hip_set_raw_batch_kernel(ctx, 0)) goes to the LDS-tile builds
static bool regBuild(const dmvio_hip_ctx* c) { return c->raw_batch_kernel && c->levels <= 4 && (c->w % 8) == 0 && (c->h % 8) == 0; }
static dim3 regGrid(const dmvio_hip_ctx* c, int B) { return dim3(((c->w / 4) * (c->h / 8) + 255) / 256, B); }

// ---- deferred attach: see dmvio_hip_ctx (internal.h) and DESIGN.md section 4.  *Held: the caller holds c->pend_mu.
// The ordinary build of the slots that still wait, from the recorded source: one launch per run of consecutive entries of the staged list (the kernel finds frame f of its
// launch at base + f * stride and its slot at slots[f], so a run is the same launch shifted), stamped with the generation the attach set aside for it, then their marks cleared.
static int flushPendingHeld(dmvio_hip_ctx* c, bool wait) {
  if (!c->n_pending.load(std::memory_order_relaxed)) return 0;
  HIPCHK(hipSetDevice(c->device));
  const dmvio_hip_ctx::PendingAttach& P = c->pend;
  for (int i = 0; i < P.B;) {
    if (c->h_pending[P.slots[i]] != i + 1) { i++; continue; }
    int j = i;
    while (j < P.B && c->h_pending[P.slots[j]] == j + 1) { c->h_pending[P.slots[j]] = 0; j++; }
    hipLaunchKernelGGL((k_build_pyramids_reg<true>), regGrid(c, j - i), dim3(256), 0, c->stream, P.base + (size_t)i * P.stride, P.stride, c->pg, c->fs_, P.d_slots + i, 0, P.flush_gen);
    hipLaunchKernelGGL(k_clear_pending, dim3((j - i + 255) / 256), dim3(256), 0, c->stream, c->fs_, P.d_slots + i, j - i);
    i = j;
  }
  c->n_pending.store(0, std::memory_order_release);
  HIPCHK(hipGetLastError());
  if (wait) HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int dmv_flush_pending_held(dmvio_hip_ctx* c) { return flushPendingHeld(c, false); }
int dmv_flush_pending(dmvio_hip_ctx* c, int wait) {
  std::lock_guard<std::mutex> pl(c->pend_mu);
  return flushPendingHeld(c, wait != 0);
}
// the host marks of slots another build is about to rewrite (the device marks follow: a memset for one slot, k_clear_pending for a staged list); returns how many waited
static int dropPendingHeld(dmvio_hip_ctx* c, int B, const int* slots) {
  if (!c->n_pending.load(std::memory_order_relaxed)) return 0;
  int n = 0;
  for (int i = 0; i < B; i++) if (c->h_pending[slots[i]]) { c->h_pending[slots[i]] = 0; n++; }
  c->n_pending.fetch_sub(n, std::memory_order_release);
  return n;
}
static int buildPyramid(dmvio_hip_ctx* c, int slot, const float* d_color) {
  {
    std::lock_guard<std::mutex> pl(c->pend_mu);
    if (dropPendingHeld(c, 1, &slot)) HIPCHK(hipMemsetAsync(c->fs_.pend_gen() + slot, 0, sizeof(unsigned int), c->stream));
  }
  hipLaunchKernelGGL(k_build_pyramids, dim3(c->pg.tiles_x * c->pg.tiles_y, 1), dim3(256), 0, c->stream, d_color, (size_t)0, c->pg, c->fs_,
                     (const int*)nullptr, slot, ++c->build_gen, 0);
  c->h_lvl0[slot] = c->fs_.own_level(slot, 0); c->h_tiled[slot] = 0;
  HIPCHK(hipGetLastError());
  return 0;
}

// see internal.h
int dmv_ensure_row_major_locked(dmvio_hip_ctx* c, int slot) {
  if (slot < 0 || slot >= c->n_slots || !c->h_tiled[slot]) return 0;
  HIPCHK(hipSetDevice(c->device));
  const int n = c->w * c->h;
  float* own = c->fs_.own_level(slot, 0);
  hipLaunchKernelGGL(k_untile_level0, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const float*)own, c->w, c->h, c->d_upload);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(own, c->d_upload, sizeof(float) * n, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemsetAsync(c->fs_.tiled0 + slot, 0, 1, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));   // consumers on other streams (a window optimiser's) read the plane next
  c->h_tiled[slot] = 0;
  return 0;
}
int dmv_ensure_row_major(dmvio_hip_ctx* c, int slot) {
  if (!c) return failmsg("null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  return dmv_ensure_row_major_locked(c, slot);
}
// What dmvio_hip_frames_from_raw_device_batch writes as level 0: 0 = row-major (default), 1 = 8x4 tiles (the coarse tracker's batch kernel reads them natively; other consumers
// convert the slot back on first use).  Tiles need w % 8 == 0 and h % 4 == 0; other sizes are always row-major.  Measured (profiles/r04_*): the tiled plane saves lines per tap
// (2.4 instead of 4.3) but costs twelve dword loads with their own tile addresses instead of four vector loads — k_track_lm 3.78 vs 3.50 ms per 4096 frames — hence not the default.
int dmvio_hip_set_raw_batch_layout(dmvio_hip_ctx* c, int tiled) {
  if (!c) return failmsg("null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  c->raw_batch_tiled = tiled ? 1 : 0;
  return 0;
}
// Which kernels build the pyramids of the raw-image batch and of frames attached in place: 1 (default) = the wave-autonomous register builds where the geometry allows it
// (at most four pyramid levels, both sides multiples of 8), 0 = always the LDS-tile builds.  Both write the same bits; the switch exists for A/B measurements and the parity test of the two.
int dmvio_hip_set_raw_batch_kernel(dmvio_hip_ctx* c, int variant) {
  if (!c) return failmsg("null ctx");
  if (variant != 0 && variant != 1) return failmsg("set_raw_batch_kernel: variant must be 0 or 1");
  std::lock_guard<std::mutex> lk(c->mu);
  c->raw_batch_kernel = variant;
  return 0;
}
// 1 (default): dmvio_hip_frames_attach_device_batch only records the attach (one small kernel) where the register build would run on the context's stream; the coarser
// levels of a slot are formed by the batched tracking kernel that first reads it (k_track_lm_build) or, for every other reader, right before that reader.  0: the attach
// launches the build itself.  Same planes, same stamps' meaning, same results either way (tests/test_track_fused_build_gpu.py).
int dmvio_hip_set_deferred_attach(dmvio_hip_ctx* c, int on) {
  if (!c) return failmsg("null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  if (int r = dmv_flush_pending(c, 0)) return r;
  c->deferred_attach = on ? 1 : 0;
  return 0;
}
int dmvio_hip_frame_level0_is_tiled(dmvio_hip_ctx* c, int slot) {
  if (!c || slot < 0 || slot >= c->n_slots) return failmsg("frame_level0_is_tiled: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  return c->h_tiled[slot] ? 1 : 0;
}

int dmvio_hip_frame_upload(dmvio_hip_ctx* c, int slot, const float* host) {
  if (!c || !host) return failmsg("frame_upload: null argument");
  if (slot < 0 || slot >= c->n_slots) return failmsg("frame_upload: slot out of range");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(c->bounce.h2d(c->d_upload, host, sizeof(float) * c->w * c->h, c->stream));   // a pageable 1 MB source costs ~0.27 ms per copy, a memcpy + a pinned copy ~0.07 ms
  if (int r = buildPyramid(c, slot, c->d_upload)) return r;
  HIPCHK(c->bounce.finish(c->stream));
  return 0;
}

// ---- raw camera image -> photometric + geometric undistortion -> pyramids (Undistort::undistort + FrameHessian::makeImages)
struct dmvio_hip_undistorter {
  dmvio_hip_ctx* ctx = nullptr;
  UndistortDev U{};
  int bytes_per_px = 1;
  float *d_G = nullptr, *d_vig = nullptr, *d_rx = nullptr, *d_ry = nullptr;
  void *d_raw = nullptr, *h_raw = nullptr;
};
dmvio_hip_undistorter* dmvio_hip_undistorter_create(dmvio_hip_ctx* c, int wOrg, int hOrg, int bits, const float* G, const float* vignetteMapInv, const float* remapX,
                                                    const float* remapY) {
  if (!c || wOrg < 1 || hOrg < 1 || (bits != 8 && bits != 16)) { failmsg("undistorter_create: bad argument"); return nullptr; }
  if ((remapX == nullptr) != (remapY == nullptr)) { failmsg("undistorter_create: remapX / remapY must both be given or both be NULL"); return nullptr; }
  if (!remapX && (wOrg != c->w || hOrg != c->h)) { failmsg("undistorter_create: passthrough needs wOrg x hOrg == w x h"); return nullptr; }
  if (remapX) {
    // the bilinear taps of a remapped pixel are (xi, yi), (xi+1, yi), (xi, yi+1), (xi+1, yi+1) of the raw image with xi = (int)x, yi = (int)y: they are in bounds
    // exactly when 0 <= x < wOrg-1 and 0 <= y < hOrg-1.  The reference's remap generation keeps 0 < x < wOrg-1, 0 < y < hOrg-1 and marks everything else with -1
    // (Undistort.cpp:920-942, "make rounding resistant"), so its tables always pass; a table that does not would read out of bounds.
    const size_t nOutChk = (size_t)c->w * c->h;
    for (size_t i = 0; i < nOutChk; i++) {
      const float x = remapX[i], y = remapY[i];
      if (x < 0) continue;
      if (!(x < (float)(wOrg - 1)) || !(y >= 0) || !(y < (float)(hOrg - 1)) || (int)x + 1 > wOrg - 1 || (int)y + 1 > hOrg - 1) {
        failmsg("undistorter_create: remap entry outside the raw image (mark invalid pixels with remapX = -1)");
        return nullptr;
      }
    }
  }
  if (hipSetDevice(c->device) != hipSuccess) { failmsg("undistorter_create: hipSetDevice failed"); return nullptr; }
  dmvio_hip_undistorter* u = new dmvio_hip_undistorter();
  u->ctx = c; u->bytes_per_px = bits / 8;
  const size_t nOrg = (size_t)wOrg * hOrg, nOut = (size_t)c->w * c->h, nG = bits == 8 ? 256 : 65536;
  bool ok = hipMalloc(&u->d_raw, nOrg * u->bytes_per_px) == hipSuccess && hipHostMalloc(&u->h_raw, nOrg * u->bytes_per_px, hipHostMallocDefault) == hipSuccess;
  auto up = [&](float** d, const float* h, size_t n) {
    if (!h) return true;
    return hipMalloc((void**)d, sizeof(float) * n) == hipSuccess && hipMemcpy(*d, h, sizeof(float) * n, hipMemcpyHostToDevice) == hipSuccess;
  };
  ok = ok && up(&u->d_G, G, nG) && up(&u->d_vig, G ? vignetteMapInv : nullptr, nOrg) && up(&u->d_rx, remapX, nOut) && up(&u->d_ry, remapY, nOut);
  if (!ok) { failmsg("undistorter_create: device allocation failed"); dmvio_hip_undistorter_destroy(u); return nullptr; }
  u->U.wOrg = wOrg; u->U.hOrg = hOrg; u->U.w = c->w; u->U.h = c->h;
  u->U.G = u->d_G; u->U.vignetteMapInv = u->d_vig; u->U.remapX = u->d_rx; u->U.remapY = u->d_ry; u->U.factor = 1.0f;
  return u;
}
void dmvio_hip_undistorter_destroy(dmvio_hip_undistorter* u) {
  if (!u) return;
  hipSetDevice(u->ctx->device);
  hipStreamSynchronize(u->ctx->stream);
  if (u->d_raw) hipFree(u->d_raw);
  if (u->h_raw) hipHostFree(u->h_raw);
  if (u->d_G) hipFree(u->d_G);
  if (u->d_vig) hipFree(u->d_vig);
  if (u->d_rx) hipFree(u->d_rx);
  if (u->d_ry) hipFree(u->d_ry);
  delete u;
}
int dmvio_hip_frame_upload_raw(dmvio_hip_ctx* c, dmvio_hip_undistorter* u, int slot, const void* raw, float factor, float* undistorted_out) {
  if (!c || !u || !raw || u->ctx != c) return failmsg("frame_upload_raw: bad argument");
  if (slot < 0 || slot >= c->n_slots) return failmsg("frame_upload_raw: slot out of range");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  const size_t nOrg = (size_t)u->U.wOrg * u->U.hOrg, nOut = (size_t)c->w * c->h;
  HIPCHK(hipStreamSynchronize(c->stream));   // the pinned staging buffer of a previous upload
  memcpy(u->h_raw, raw, nOrg * u->bytes_per_px);
  HIPCHK(hipMemcpyAsync(u->d_raw, u->h_raw, nOrg * u->bytes_per_px, hipMemcpyHostToDevice, c->stream));
  UndistortDev U = u->U;
  U.factor = factor;
  if (u->bytes_per_px == 1) hipLaunchKernelGGL((k_undistort<unsigned char>), dim3((nOut + 255) / 256), dim3(256), 0, c->stream, (const unsigned char*)u->d_raw, U, c->d_upload);
  else hipLaunchKernelGGL((k_undistort<unsigned short>), dim3((nOut + 255) / 256), dim3(256), 0, c->stream, (const unsigned short*)u->d_raw, U, c->d_upload);
  HIPCHK(hipGetLastError());
  if (int r = buildPyramid(c, slot, c->d_upload)) return r;
  if (undistorted_out) HIPCHK(c->bounce.d2h(undistorted_out, c->d_upload, sizeof(float) * nOut, c->stream));
  HIPCHK(c->bounce.finish(c->stream));
  return 0;
}

int dmvio_hip_frame_from_device(dmvio_hip_ctx* c, int slot, const float* dev) {
  if (!c || !dev) return failmsg("frame_from_device: null argument");
  if (slot < 0 || slot >= c->n_slots) return failmsg("frame_from_device: slot out of range");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  return buildPyramid(c, slot, dev);  // asynchronous on the ctx stream
}

// slot list of a batched build -> device (kept while the same list comes again); caller holds c->mu and c->pend_mu
static int stageSlots(dmvio_hip_ctx* c, int B, const int* slots) {
  for (int i = 0; i < B; i++) if (slots[i] < 0 || slots[i] >= c->n_slots) return failmsg("frame batch: slot out of range");
  dmvio_hip_ctx::SlotList* hit = nullptr;
  dmvio_hip_ctx::SlotList* lru = &c->slot_lists[0];
  for (auto& L : c->slot_lists) {
    if (L.n == B && L.h && !memcmp(L.h, slots, sizeof(int) * B)) { hit = &L; break; }
    if (L.used < lru->used) lru = &L;
  }
  if (!hit) {
    hit = lru;
    if (hit->d && hit->d == c->pend.d_slots) { if (int r = flushPendingHeld(c, false)) return r; }   // slots that still wait are listed in the entry about to be rewritten
    // the pinned copy may still be the source of an in-flight upload, the device copy the argument of a running build: drain before rewriting
    HIPCHK(hipStreamSynchronize(buildStream(c)));
    if (c->build_stream) HIPCHK(hipStreamSynchronize(c->stream));
    if (B > hit->cap) {
      if (hit->d) { HIPCHK(hipFree(hit->d)); HIPCHK(hipHostFree(hit->h)); hit->d = nullptr; hit->h = nullptr; }
      hit->cap = std::max(B, 64);
      HIPCHK(hipMalloc((void**)&hit->d, sizeof(int) * hit->cap));
      HIPCHK(hipHostMalloc((void**)&hit->h, sizeof(int) * hit->cap, hipHostMallocDefault));
    }
    memcpy(hit->h, slots, sizeof(int) * B);
    hit->n = B;
    HIPCHK(hipMemcpyAsync(hit->d, hit->h, sizeof(int) * B, hipMemcpyHostToDevice, buildStream(c)));
  }
  hit->used = ++c->slot_clock;
  c->d_slots = hit->d;
  return 0;
}

static int framesFromDeviceBatch(dmvio_hip_ctx* c, int B, const int* slots, const float* dev_base, size_t stride_bytes, const bool attach) {
  if (!c || !slots || !dev_base) return failmsg("frames_from_device_batch: null argument");
  if (B <= 0 || stride_bytes % sizeof(float)) return failmsg("frames_from_device_batch: bad B / stride");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < B; i++) if (slots[i] < 0 || slots[i] >= c->n_slots) return failmsg("frame batch: slot out of range");
  std::lock_guard<std::mutex> pl(c->pend_mu);
  // slots of this call that still wait for a deferred build are superseded: their old image is never read
  const int dropped = dropPendingHeld(c, B, slots);
  if (int r = stageSlots(c, B, slots)) return r;
  if (attach && regBuild(c) && !c->build_stream && c->deferred_attach) {
    // deferred: only the table kernel now; the levels 1.. are formed by the tracking kernel that first reads a slot, or by a flush.  One deferred attach is kept: what an
    // older one left is built first.  Three generations: "not known clean" until built, the stamp of a build inside the tracking kernel, the stamp of a flush.
    if (int r = flushPendingHeld(c, false)) return r;
    const unsigned int gen = c->build_gen + 1u;
    c->build_gen += 3u;
    hipLaunchKernelGGL(k_attach_deferred, dim3((B + 255) / 256), dim3(256), 0, c->stream, dev_base, stride_bytes / sizeof(float), c->fs_, (const int*)c->d_slots, B, gen);
    dmvio_hip_ctx::PendingAttach& P = c->pend;
    P.base = dev_base; P.stride = stride_bytes / sizeof(float); P.d_slots = c->d_slots; P.B = B; P.flush_gen = gen + 2u;
    P.slots.assign(slots, slots + B);
    int n = 0;
    for (int i = 0; i < B; i++) { if (!c->h_pending[slots[i]]) n++; c->h_pending[slots[i]] = i + 1; }
    c->n_pending.store(n, std::memory_order_release);
    for (int i = 0; i < B; i++) { c->h_lvl0[slots[i]] = dev_base + (size_t)i * P.stride; c->h_tiled[slots[i]] = 0; }
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (dropped) hipLaunchKernelGGL(k_clear_pending, dim3((B + 255) / 256), dim3(256), 0, c->stream, c->fs_, (const int*)c->d_slots, B);
  // attached in place: the register build (read-dominated: 5 % ahead); level 0 copied: the LDS-tile build (4 % ahead there) — both measured, tools/time_pyramids.py
  if (regBuild(c) && attach)
    hipLaunchKernelGGL((k_build_pyramids_reg<true>), regGrid(c, B), dim3(256), 0, buildStream(c), dev_base, stride_bytes / sizeof(float), c->pg, c->fs_, (const int*)c->d_slots, 0, ++c->build_gen);
  else
    hipLaunchKernelGGL(k_build_pyramids, dim3(c->pg.tiles_x * c->pg.tiles_y, B), dim3(256), 0, buildStream(c), dev_base, stride_bytes / sizeof(float),
                       c->pg, c->fs_, (const int*)c->d_slots, 0, ++c->build_gen, attach ? 1 : 0);
  for (int i = 0; i < B; i++) { c->h_lvl0[slots[i]] = attach ? dev_base + (size_t)i * (stride_bytes / sizeof(float)) : c->fs_.own_level(slots[i], 0); c->h_tiled[slots[i]] = 0; }
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
// the eight instantiations of the raw-image builds: pixel type (the caller), then register / LDS-tile build x tiled / row-major level 0
template <typename T>
static void launchRawBuild(dmvio_hip_ctx* c, bool reg, bool tiled, dim3 grid, const void* raw, size_t stride, const UndistortDev& U) {
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, buildStream(c), (const T*)raw, stride, U, c->pg, c->fs_, (const int*)c->d_slots, ++c->build_gen); };
  if (reg) { if (tiled) go(k_build_pyramids_raw_reg<T, true>); else go(k_build_pyramids_raw_reg<T, false>); }
  else { if (tiled) go(k_build_pyramids_raw<T, true>); else go(k_build_pyramids_raw<T, false>); }
}
extern "C" {

// B raw camera images already on the device (the caller's own pinned buffers / copy stream brought them there, 1 or 2 bytes per pixel) -> undistorted level 0
// + pyramids of B slots in one launch; asynchronous on the ctx stream like the fp32 variants.  Undistort::undistort + FrameHessian::makeImages per frame.
int dmvio_hip_frames_from_raw_device_batch(dmvio_hip_ctx* c, dmvio_hip_undistorter* u, int B, const int* slots, const void* raw_dev_base, size_t stride_bytes, float factor) {
  if (!c || !u || !slots || !raw_dev_base || u->ctx != c) return failmsg("frames_from_raw_device_batch: bad argument");
  const size_t nOrg = (size_t)u->U.wOrg * u->U.hOrg;
  if (B <= 0 || stride_bytes % u->bytes_per_px || stride_bytes < nOrg * u->bytes_per_px || (uintptr_t)raw_dev_base % u->bytes_per_px)
    return failmsg("frames_from_raw_device_batch: bad B / stride / alignment");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < B; i++) if (slots[i] < 0 || slots[i] >= c->n_slots) return failmsg("frame batch: slot out of range");
  std::lock_guard<std::mutex> pl(c->pend_mu);
  const int dropped = dropPendingHeld(c, B, slots);   // rewritten here: a deferred build of these slots is void
  if (int r = stageSlots(c, B, slots)) return r;
  if (dropped) hipLaunchKernelGGL(k_clear_pending, dim3((B + 255) / 256), dim3(256), 0, c->stream, c->fs_, (const int*)c->d_slots, B);
  UndistortDev U = u->U;
  U.factor = factor;
  // level 0 in 8x4 tiles on request (dmvio_hip_set_raw_batch_layout)
  const bool tiled = c->raw_batch_tiled && (c->w % 8) == 0 && (c->h % 4) == 0;
  // the wave-autonomous build (a 4 x 8 pixel block per thread, levels in registers) where the pyramid allows it, the LDS-tile build otherwise
  const bool reg = regBuild(c);
  const dim3 grid = reg ? regGrid(c, B) : dim3(c->pg.tiles_x * c->pg.tiles_y, B);
  if (u->bytes_per_px == 1) launchRawBuild<unsigned char>(c, reg, tiled, grid, raw_dev_base, stride_bytes, U);
  else launchRawBuild<unsigned short>(c, reg, tiled, grid, raw_dev_base, stride_bytes / 2, U);
  for (int i = 0; i < B; i++) { c->h_lvl0[slots[i]] = c->fs_.own_level(slots[i], 0); c->h_tiled[slots[i]] = tiled ? 1 : 0; }
  HIPCHK(hipGetLastError());
  return 0;
}

int dmvio_hip_frames_from_device_batch(dmvio_hip_ctx* c, int B, const int* slots, const float* dev_base, size_t stride_bytes) {
  return framesFromDeviceBatch(c, B, slots, dev_base, stride_bytes, false);
}
// Zero-copy variant: the intensity plane of level 0 IS the caller's image (this library stores no gradient channels), so only the coarser
// levels are built; the slots reference dev_base until they are rebuilt, and the caller keeps those images valid and unchanged meanwhile.
int dmvio_hip_frames_attach_device_batch(dmvio_hip_ctx* c, int B, const int* slots, const float* dev_base, size_t stride_bytes) {
  return framesFromDeviceBatch(c, B, slots, dev_base, stride_bytes, true);
}

// Diagnostics: withdraw the "every pixel finite" stamp of a slot, so that its consumers take the guarded code path (tests compare the two)
int dmvio_hip_frame_mark_unclean(dmvio_hip_ctx* c, int slot) {
  if (!c || slot < 0 || slot >= c->n_slots) return failmsg("frame_mark_unclean: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  if (int r = dmv_flush_pending(c, 0)) return r;
  HIPCHK(hipMemcpyAsync(c->fs_.bad_gen + slot, c->fs_.build_gen + slot, sizeof(unsigned int), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// Diagnostics: 1 when the slot's last build stamped it clean (every pixel finite, |I| <= 1e30), 0 when not, < 0 on error.  Waits for the context's stream.
int dmvio_hip_frame_is_clean(dmvio_hip_ctx* c, int slot) {
  if (!c || slot < 0 || slot >= c->n_slots) return failmsg("frame_is_clean: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  if (int r = dmv_flush_pending(c, 0)) return r;   // the verdict of a slot that still waits is formed with its levels
  unsigned int g[2] = {0, 0};
  HIPCHK(c->bounce.d2h(&g[0], c->fs_.build_gen + slot, sizeof(unsigned int), c->stream));
  HIPCHK(c->bounce.d2h(&g[1], c->fs_.bad_gen + slot, sizeof(unsigned int), c->stream));
  HIPCHK(c->bounce.finish(c->stream));
  return g[0] != g[1] ? 1 : 0;
}

int dmvio_hip_frame_download(dmvio_hip_ctx* c, int slot, int lvl, float* out) {
  if (!c || !out) return failmsg("frame_download: null argument");
  if (slot < 0 || slot >= c->n_slots || lvl < 0 || lvl >= c->levels) return failmsg("frame_download: out of range");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  const int n = c->wl[lvl] * c->hl[lvl];
  if (lvl == 0) { if (int r = dmv_ensure_row_major_locked(c, slot)) return r; }
  hipLaunchKernelGGL(k_level_to_f3, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->levelPtr(slot, lvl), c->wl[lvl], c->hl[lvl], c->d_f3);
  HIPCHK(hipGetLastError());
  HIPCHK(c->bounce.d2h(out, c->d_f3, sizeof(float) * 3 * n, c->stream));
  HIPCHK(c->bounce.finish(c->stream));
  return 0;
}

// FrameHessian::makeImages' absSquaredGrad planes (the input of PixelSelector::makeMaps / makeHists) of a resident frame
int dmvio_hip_frame_abs_squared_grad(dmvio_hip_ctx* c, int slot, int n_levels, const float* B_lut256, float* const* out_host) {
  if (!c || !out_host) return failmsg("frame_abs_squared_grad: null argument");
  if (slot < 0 || slot >= c->n_slots || n_levels < 1 || n_levels > c->levels) return failmsg("frame_abs_squared_grad: out of range");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  if (int r = dmv_ensure_row_major_locked(c, slot)) return r;
  // scratch layout inside d_f3 (3*w*h floats): [256-entry response table | level 0 | level 1 | ...]  (sum of the levels < 1.34 w*h)
  float* d_lut = nullptr;
  float* d_out = c->d_f3 + 256;
  if ((size_t)256 + (size_t)c->wl[0] * c->hl[0] * 4 / 3 + 16 > (size_t)3 * c->wl[0] * c->hl[0]) return failmsg("frame_abs_squared_grad: frame too small");
  if (B_lut256) {
    d_lut = c->d_f3;
    HIPCHK(c->bounce.h2d(d_lut, B_lut256, sizeof(float) * 256, c->stream));
  }
  size_t off = 0;
  for (int l = 0; l < n_levels; l++) {
    const int n = c->wl[l] * c->hl[l];
    hipLaunchKernelGGL(k_abs_squared_grad, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->levelPtr(slot, l), c->wl[l], c->hl[l], (const float*)d_lut, d_out + off);
    if (out_host[l]) HIPCHK(c->bounce.d2h(out_host[l], d_out + off, sizeof(float) * n, c->stream));
    off += n;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(c->bounce.finish(c->stream));
  return 0;
}

// FullSystem::printResult (FullSystem.cpp:256-298): one line "timestamp tx ty tz qx qy qz qw" per frame with a valid pose, 15
// significant digits, poses relative to the first frame (camToFirst = firstPose^-1 * camToWorld); frames that are not keyframes are
// re-based on their tracking reference's CURRENT pose when tracking_ref / camToTrackingRef7 are given (useCamToTrackingRef).
// Host-only (no device work): the on-disk edge of the path, so that trajectories of both pipelines compare file against file.
int dmvio_hip_write_result_txt(const char* path, int n, const double* timestamps, const double* camToWorld7, const unsigned char* pose_valid,
                               const int* tracking_ref, const double* camToTrackingRef7, const double firstPose7[7]) {
  if (!path || n < 0 || (n > 0 && (!timestamps || !camToWorld7)) || !firstPose7) return failmsg("write_result_txt: bad argument");
  if (tracking_ref && !camToTrackingRef7) return failmsg("write_result_txt: tracking_ref without camToTrackingRef7");
  FILE* f = fopen(path, "w");
  if (!f) return failmsg("write_result_txt: cannot open the file");
  const Pose firstInv = poseInv(poseFrom7(firstPose7));
  for (int i = 0; i < n; i++) {
    if (pose_valid && !pose_valid[i]) continue;
    Pose c2w = poseFrom7(camToWorld7 + 7 * i);
    if (tracking_ref && tracking_ref[i] >= 0) {
      if (tracking_ref[i] >= n) { fclose(f); return failmsg("write_result_txt: tracking_ref out of range"); }
      c2w = poseMul(poseFrom7(camToWorld7 + 7 * tracking_ref[i]), poseFrom7(camToTrackingRef7 + 7 * i));
    }
    double p[7];
    poseTo7(poseMul(firstInv, c2w), p);
    fprintf(f, "%.15g %.15g %.15g %.15g %.15g %.15g %.15g %.15g\n", timestamps[i], p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
  }
  if (fclose(f) != 0) return failmsg("write_result_txt: write failed");
  return 0;
}

}  // extern "C"
