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

#define DMV_FRAME_STORE_IMPL   // this unit compiles the frame store's function bodies (frame_store_host.hpp): they launch kernels of image_kernels.hpp
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
  c->pg.levels = c->levels;
  for (int l = 0; l < c->levels; l++) { c->pg.w[l] = c->wl[l] = w >> l; c->pg.h[l] = c->hl[l] = h >> l; }
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  if (int r = c->frames.init(c->device, n_frame_slots)) return r;
  HIPCHK(hipMalloc((void**)&c->d_upload, sizeof(float) * w * h));
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
  if (c->stream) hipStreamSynchronize(c->stream);   // (null only in a handle whose creation failed)
  c->frames.release();
  dmvInitLmRelease(c);
  hipFree(c->d_upload);
  c->bounce.release();
  hipFree(c->d_f3);
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
  delete c;
}

int dmvio_hip_pyr_levels(const dmvio_hip_ctx* c) { return c ? c->levels : 0; }

int dmvio_hip_set_stream(dmvio_hip_ctx* c, void* s) {
  if (!c) return failmsg("null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  if (int r = c->frames.flush(false)) return r;   // a deferred attach is finished on the stream it was made on
  HIPCHK(hipStreamSynchronize(c->stream));
  if (s) {
    if (c->own_stream) { HIPCHK(hipStreamDestroy(c->stream)); }
    c->stream = (hipStream_t)s; c->own_stream = false;
  } else if (!c->own_stream) {
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true;
  }
  return 0;
}

// The stream the BATCHED pyramid builds (dmvio_hip_frames_from_device_batch / _attach_device_batch / _from_raw_device_batch) are enqueued on; NULL (default): the context's
// stream.  With a stream of its own the build of batch k+1 overlaps the tracking of batch k — the build is bound by HBM, k_track_lm by its L1 miss path and VALU issue.  The
// CALLER orders the two streams (events): a build must not start before the consumers of the slots it rewrites have finished, a consumer not before the build of its slots.
int dmvio_hip_set_build_stream(dmvio_hip_ctx* c, void* s) {
  if (!c) return failmsg("null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  if (int r = c->frames.flush(false)) return r;   // with a build stream nothing is deferred: what waits is built now, on the context's stream
  HIPCHK(hipStreamSynchronize(c->frames.buildStream()));
  c->frames.build_stream = (hipStream_t)s;
  return 0;
}

int dmvio_hip_synchronize(dmvio_hip_ctx* c) {
  if (!c) return failmsg("null ctx");
  HIPCHK(hipSetDevice(c->device));
  if (int r = c->frames.flush(false)) return r;   // after a synchronize every slot is built: the caller may read the store from any stream
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->frames.build_stream) HIPCHK(hipStreamSynchronize(c->frames.build_stream));
  return 0;
}

// ------------------------------------------------------------------ frames
// the wave-autonomous builds (a 4 x 8 pixel block per thread, levels in registers: image_kernels.hpp) take pyramids of at most four levels on images whose sides are
// multiples of 8; everything else (and dmvio_hip_set_raw_batch_kernel(ctx, 0)) goes to the LDS-tile builds
static bool regBuild(const dmvio_hip_ctx* c) { return c->raw_batch_kernel && c->levels <= 4 && (c->w % 8) == 0 && (c->h % 8) == 0; }
static int buildPyramid(dmvio_hip_ctx* c, int slot, const float* d_color) {
  unsigned int gen;
  if (int r = c->frames.begin_locked(1, &slot, nullptr, &gen)) return r;
  hipLaunchKernelGGL(k_build_pyramids, dim3(c->pg.tiles_x * c->pg.tiles_y, 1), dim3(256), 0, c->stream, d_color, (size_t)0, c->pg, c->frames.as_is(), (const int*)nullptr, slot, gen, 0);
  c->frames.commit_locked(1, &slot, nullptr, 0, false);
  HIPCHK(hipGetLastError());
  return 0;
}

// see internal.h
int dmv_ensure_row_major_locked(dmvio_hip_ctx* c, int slot) {
  if (slot < 0 || slot >= c->n_slots || !c->frames.is_tiled(slot)) return 0;
  HIPCHK(hipSetDevice(c->device));
  const int n = c->w * c->h; float* own = c->frames.as_is().own_level(slot, 0);
  hipLaunchKernelGGL(k_untile_level0, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const float*)own, c->w, c->h, c->d_upload);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(own, c->d_upload, sizeof(float) * n, hipMemcpyDeviceToDevice, c->stream));
  return c->frames.untiled_locked(slot);
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
  c->raw_batch_layout = tiled ? 1 : 0;
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
  if (int r = c->frames.flush(false)) return r;
  c->frames.deferred_attach = on ? 1 : 0;
  return 0;
}
int dmvio_hip_frame_level0_is_tiled(dmvio_hip_ctx* c, int slot) {
  if (!c || slot < 0 || slot >= c->n_slots) return failmsg("frame_level0_is_tiled: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  return c->frames.is_tiled(slot) ? 1 : 0;
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

static int framesFromDeviceBatch(dmvio_hip_ctx* c, int B, const int* slots, const float* dev_base, size_t stride_bytes, const bool attach) {
  if (!c || !slots || !dev_base) return failmsg("frames_from_device_batch: null argument");
  if (B <= 0 || stride_bytes % sizeof(float)) return failmsg("frames_from_device_batch: bad B / stride");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  FrameSlots& F = c->frames;
  const size_t stride = stride_bytes / sizeof(float);
  // deferred: where the register build would run on the context's stream, and the switch is on
  if (attach && regBuild(c) && !F.build_stream && F.deferred_attach) return F.defer_locked(B, slots, dev_base, stride);
  const int* d_slots; unsigned int gen;
  if (int r = F.begin_locked(B, slots, &d_slots, &gen)) return r;
  // attached in place: the register build (read-dominated: 5 % ahead); level 0 copied: the LDS-tile build (4 % ahead there) — both measured, tools/time_pyramids.py
  if (regBuild(c) && attach)
    hipLaunchKernelGGL((k_build_pyramids_reg<true>), F.regGrid(B), dim3(256), 0, F.buildStream(), dev_base, stride, c->pg, F.as_is(), d_slots, 0, gen);
  else
    hipLaunchKernelGGL(k_build_pyramids, dim3(c->pg.tiles_x * c->pg.tiles_y, B), dim3(256), 0, F.buildStream(), dev_base, stride, c->pg, F.as_is(), d_slots, 0, gen, attach ? 1 : 0);
  F.commit_locked(B, slots, attach ? dev_base : nullptr, stride, false);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
// the eight instantiations of the raw-image builds: pixel type (the caller), then register / LDS-tile build x tiled / row-major level 0
template <typename T>
static void launchRawBuild(dmvio_hip_ctx* c, bool reg, bool tiled, dim3 grid, const void* raw, size_t stride, const UndistortDev& U, const int* d_slots, unsigned int gen) {
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->frames.buildStream(), (const T*)raw, stride, U, c->pg, c->frames.as_is(), d_slots, gen); };
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
  const int* d_slots; unsigned int gen;
  if (int r = c->frames.begin_locked(B, slots, &d_slots, &gen)) return r;
  UndistortDev U = u->U;
  U.factor = factor;
  // level 0 in 8x4 tiles on request (dmvio_hip_set_raw_batch_layout)
  const bool tiled = c->raw_batch_layout && (c->w % 8) == 0 && (c->h % 4) == 0;
  // the wave-autonomous build (a 4 x 8 pixel block per thread, levels in registers) where the pyramid allows it, the LDS-tile build otherwise
  const bool reg = regBuild(c);
  const dim3 grid = reg ? c->frames.regGrid(B) : dim3(c->pg.tiles_x * c->pg.tiles_y, B);
  if (u->bytes_per_px == 1) launchRawBuild<unsigned char>(c, reg, tiled, grid, raw_dev_base, stride_bytes, U, d_slots, gen);
  else launchRawBuild<unsigned short>(c, reg, tiled, grid, raw_dev_base, stride_bytes / 2, U, d_slots, gen);
  c->frames.commit_locked(B, slots, nullptr, 0, tiled);
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
  if (int r = c->frames.flush(false)) return r;
  HIPCHK(hipMemcpyAsync(c->frames.as_is().bad_gen + slot, c->frames.as_is().build_gen + slot, sizeof(unsigned int), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// Diagnostics: 1 when the slot's last build stamped it clean (every pixel finite, |I| <= 1e30), 0 when not, < 0 on error.  Waits for the context's stream.
int dmvio_hip_frame_is_clean(dmvio_hip_ctx* c, int slot) {
  if (!c || slot < 0 || slot >= c->n_slots) return failmsg("frame_is_clean: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  if (int r = c->frames.flush(false)) return r;   // the verdict of a slot that still waits is formed with its levels
  unsigned int g[2] = {0, 0};
  HIPCHK(c->bounce.d2h(&g[0], c->frames.as_is().build_gen + slot, sizeof(unsigned int), c->stream));
  HIPCHK(c->bounce.d2h(&g[1], c->frames.as_is().bad_gen + slot, sizeof(unsigned int), c->stream));
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
  hipLaunchKernelGGL(k_level_to_f3, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->frames.levelPtr(slot, lvl), c->wl[lvl], c->hl[lvl], c->d_f3);
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
    hipLaunchKernelGGL(k_abs_squared_grad, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->frames.levelPtr(slot, l), c->wl[l], c->hl[l], (const float*)d_lut, d_out + off);
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
