// The host side of the frame store (dmv::FrameStore, common.h): FrameSlots, a member of dmvio_hip_ctx, owns the per-slot state and writes every transition once.  A slot is
//   on its own plane, row-major | on its own plane in 8x4 tiles | attached and built | attached and WAITING for its coarser levels (a deferred attach).
// A waiting slot is built by the tracker's batch kernel (claimWaiting_locked), by a flush (flush, the readers) or is superseded by a rewrite (begin_locked, defer_locked).
// Locking.  `_locked`: the caller holds the context's `mu`; the level-0 mirror, the layout flags, the generation counter and the staged lists change only there.  The waiting
// marks, their count and the recorded attach are under pend_mu, a leaf lock private to this class: taken after `mu` by the _locked functions and alone by flush() and the
// readers, which the window optimisers' threads call without `mu`.  The count is atomic: a reader pays one load when nothing waits.
// Included by internal.h (needs its failmsg / HIPCHK); the bodies that launch kernels of image_kernels.hpp are compiled by capi_frames.hip alone (DMV_FRAME_STORE_IMPL).
#pragma once
struct FrameSlots {
  FrameSlots(const hipStream_t& ctx_stream, const dmv::PyrGeom& ctx_pg) : stream(ctx_stream), pg(ctx_pg) {}
  int deferred_attach = 1;              // dmvio_hip_set_deferred_attach
  hipStream_t build_stream = nullptr;   // dmvio_hip_set_build_stream: where the batched builds are enqueued (NULL: the context's stream)
  hipStream_t buildStream() const { return build_stream ? build_stream : stream; }
  dim3 regGrid(int B) const { return dim3(((pg.w[0] / 4) * (pg.h[0] / 8) + 255) / 256, B); }   // the register builds: a 4 x 8 pixel block per thread
  int init(int device, int n_slots);   // the device arrays, cleared on the context's stream, every slot on its own row-major plane; the geometry (pg) is set
  void release() {   // (slots that still wait are not built: nothing can read them any more, and their images need not outlive the context)
    hipFree(fs.base); hipFree(fs.build_gen); hipFree(fs.lvl0); hipFree(fs.tiled0);
    for (auto& L : slot_lists) { if (L.d) hipFree(L.d); if (L.h) hipHostFree(L.h); }
  }
  // ---- readers: the store as kernels take it.  (Known: the first two swallow the return value of a failed flush.)
  // every slot built and the context's stream waited for: any thread, no lock needed (the window optimisers and everything else that goes on on a stream of its own)
  const dmv::FrameStore& built_and_waited() { flush(true); return fs; }
  // every slot built by what is already on the context's stream: for a caller that enqueues there next (the tracker's launches other than its batch launch)
  const dmv::FrameStore& built_on_stream() { flush(false); return fs; }
  // waiting slots stay waiting: the tracker's batch launch after claimWaiting_locked / flush, and entry points that only read the device arrays' addresses
  const dmv::FrameStore& as_is() const { return fs; }
  const float* levelPtr(int slot, int lvl) { const dmv::FrameStore& s = built_and_waited(); return lvl == 0 ? slots[slot].lvl0 : s.own_level(slot, lvl); }   // as built_and_waited()
  bool is_tiled(int slot) const { return slots[slot].tiled != 0; }   // caller holds `mu`
  // the ordinary build of the slots that still wait, from the recorded source on the context's stream, which is waited for on request; any thread; 0 or <0
  int flush(bool wait) { if (!n_waiting.load(std::memory_order_acquire)) return 0; std::lock_guard<std::mutex> pl(pend_mu); return flushHeld(wait); }
  // ---- rewrites (frame_upload, frame_from_device, the copying batch build, the immediate attach, the raw-image batch): begin_locked validates the slots, withdraws the marks
  // of those that wait (their old image is never read), stages the list (d_list == NULL: one slot, nothing staged) and enqueues the device-side clear; the caller launches its
  // build with *gen; commit_locked sets the level-0 mirror (src == NULL: the slots' own planes; else frame i is the caller's image at src + i * stride) and the layout flag.
  int begin_locked(int B, const int* list, const int** d_list, unsigned int* gen) {
    std::lock_guard<std::mutex> pl(pend_mu);
    if (int r = supersedeHeld(B, list, d_list != nullptr, true)) return r;
    if (d_list) *d_list = cur->d;
    *gen = ++build_gen;
    return 0;
  }
  void commit_locked(int B, const int* list, const float* src, size_t stride, bool tiled) {
    for (int i = 0; i < B; i++) { Slot& s = slots[list[i]]; s.lvl0 = src ? src + (size_t)i * stride : fs.own_level(list[i], 0); s.tiled = tiled ? 1 : 0; }
  }
  // A deferred attach: only the table kernel now; the levels 1.. are formed by the tracking kernel that first reads a slot, or by a flush.  One deferred attach is kept:
  // what an older one left is built first.  Three generations: "not known clean" until built, the stamp of a build inside the tracking kernel, the stamp of a flush.
  int defer_locked(int B, const int* list, const float* base, size_t stride);
  // dmv_ensure_row_major_locked has converted the plane: device flag, wait (consumers on other streams read the plane next), host flag
  int untiled_locked(int slot) { HIPCHK(hipMemsetAsync(fs.tiled0 + slot, 0, 1, stream)); HIPCHK(hipStreamSynchronize(stream)); slots[slot].tiled = 0; return 0; }
  // The tracker's batch launch, whose kernel builds the waiting slots it names itself: how many of slot_of(0 .. B-1) wait, their marks withdrawn (the launch must be the
  // next thing on the stream) — unless a waiting slot is named twice (two workgroups would build and read the same planes) or none waits: then everything that waits is
  // built first and 0 returned.  Waiting slots that a claiming launch does not name stay as they are.  <0: error.
  template <class SlotOf> int claimWaiting_locked(int B, SlotOf slot_of) {
    if (!n_waiting.load(std::memory_order_acquire)) return 0;
    std::lock_guard<std::mutex> pl(pend_mu);
    int n = 0;
    for (int i = 0; i < B; i++) {   // a mark is negated where the launch names its slot first: a negative one met again is a slot named twice
      int& m = slots[slot_of(i)].waiting;
      if (m < 0) { n = 0; break; }
      if (m > 0) { m = -m; n++; }
    }
    for (int i = 0; i < B; i++) { int& m = slots[slot_of(i)].waiting; if (m < 0) m = n ? 0 : -m; }
    if (!n) return flushHeld(false);
    n_waiting.fetch_sub(n, std::memory_order_release);
    return n;
  }

 private:
  const hipStream_t& stream;   // the context's
  const dmv::PyrGeom& pg;
  int device = 0, n_slots = 0;
  dmv::FrameStore fs{};
  // lvl0, tiled: host mirror of FrameStore::lvl0 / ::tiled0.  waiting: 1 + the slot's index in the recorded attach's list, 0 = built.
  struct Slot { const float* lvl0 = nullptr; int waiting = 0; unsigned char tiled = 0; };
  std::vector<Slot> slots;
  unsigned int build_gen = 0;   // generation counter of pyramid builds (FrameStore::build_gen / bad_gen / pend_gen stamps)
  // slot lists of the batched builds, staged on the device (d) from a pinned copy (h): the last few distinct lists stay (a double-buffered pipeline alternates between two)
  struct SlotList { int *d = nullptr, *h = nullptr; int cap = 0, n = 0; unsigned long long used = 0; } slot_lists[4], *cur = nullptr;   // cur: the list of the current batched build
  unsigned long long slot_clock = 0;
  // the one deferred attach that can be outstanding: its source, its staged list (which stays while a slot of it waits) and the generation a flush stamps its slots with
  struct PendingAttach { const float* base = nullptr; size_t stride = 0; const SlotList* list = nullptr; unsigned int flush_gen = 0; } pend;
  std::atomic<int> n_waiting{0}; std::mutex pend_mu;   // how many slots wait; the lock of the marks, the count and `pend`
  // *Held: the caller holds pend_mu
  int flushHeld(bool wait);
  int supersedeHeld(int B, const int* list, bool stage, bool clear);
  int stageHeld(int B, const int* list);
};
#ifdef DMV_FRAME_STORE_IMPL
int FrameSlots::init(int device_, int n) {
  device = device_; n_slots = n;
  auto zeroed = [&](void** p, size_t bytes) { const hipError_t e = hipMalloc(p, bytes); return e != hipSuccess ? e : hipMemsetAsync(*p, 0, bytes, stream); };
  size_t off = 0;
  for (int l = 0; l < pg.levels; l++) { fs.level_off[l] = off; off += (size_t)pg.w[l] * pg.h[l]; }
  fs.levels = pg.levels; fs.slot_stride = (off + 63) & ~(size_t)63;
  HIPCHK(zeroed((void**)&fs.base, sizeof(float) * fs.slot_stride * n));
  HIPCHK(zeroed((void**)&fs.build_gen, sizeof(unsigned int) * 3 * n));   // build_gen | bad_gen: equal (0) = not known to be clean | pend_gen: 0 = built
  HIPCHK(zeroed((void**)&fs.tiled0, n));
  fs.bad_gen = fs.build_gen + n;
  HIPCHK(hipMalloc((void**)&fs.lvl0, sizeof(const float*) * n));
  slots.assign(n, Slot()); std::vector<const float*> own(n);
  for (int s = 0; s < n; s++) own[s] = slots[s].lvl0 = fs.own_level(s, 0);
  HIPCHK(hipMemcpy(fs.lvl0, own.data(), sizeof(const float*) * n, hipMemcpyHostToDevice));
  return 0;
}
// one launch per run of consecutive entries of the recorded list (the kernel finds frame f of its launch at base + f * stride and its slot at slots[f], so a run is the
// same launch shifted), stamped with the generation the attach set aside for it, then their device marks cleared
int FrameSlots::flushHeld(bool wait) {
  if (!n_waiting.load(std::memory_order_relaxed)) return 0;
  HIPCHK(hipSetDevice(device));
  const PendingAttach& P = pend; const SlotList& L = *P.list;
  for (int i = 0; i < L.n;) {
    if (slots[L.h[i]].waiting != i + 1) { i++; continue; }
    int j = i; while (j < L.n && slots[L.h[j]].waiting == j + 1) { slots[L.h[j]].waiting = 0; j++; }
    hipLaunchKernelGGL((dmv::k_build_pyramids_reg<true>), regGrid(j - i), dim3(256), 0, stream, P.base + (size_t)i * P.stride, P.stride, pg, fs, (const int*)L.d + i, 0, P.flush_gen);
    hipLaunchKernelGGL(dmv::k_clear_pending, dim3((j - i + 255) / 256), dim3(256), 0, stream, fs, (const int*)L.d + i, j - i);
    i = j;
  }
  n_waiting.store(0, std::memory_order_release); HIPCHK(hipGetLastError());
  if (wait) HIPCHK(hipStreamSynchronize(stream));
  return 0;
}
// the head of every rewrite: the one slot-range check, host marks withdrawn, the list staged if wanted, device marks cleared if wanted and any was set (no list: one slot)
int FrameSlots::supersedeHeld(int B, const int* list, bool stage, bool clear) {
  for (int i = 0; i < B; i++) if (list[i] < 0 || list[i] >= n_slots) return failmsg("frame batch: slot out of range");
  int n = 0;
  if (n_waiting.load(std::memory_order_relaxed)) {
    for (int i = 0; i < B; i++) if (slots[list[i]].waiting) { slots[list[i]].waiting = 0; n++; }
    n_waiting.fetch_sub(n, std::memory_order_release);
  }
  if (stage) { if (int r = stageHeld(B, list)) return r; }
  if (n && clear && stage) hipLaunchKernelGGL(dmv::k_clear_pending, dim3((B + 255) / 256), dim3(256), 0, stream, fs, (const int*)cur->d, B);
  else if (n && clear) HIPCHK(hipMemsetAsync(fs.pend_gen() + list[0], 0, sizeof(unsigned int), stream));
  return 0;
}
// slot list of a batched build -> device (kept while the same list comes again)
int FrameSlots::stageHeld(int B, const int* list) {
  SlotList *hit = nullptr, *lru = &slot_lists[0];
  for (auto& L : slot_lists) {
    if (L.n == B && L.h && !memcmp(L.h, list, sizeof(int) * B)) { hit = &L; break; }
    if (L.used < lru->used) lru = &L;
  }
  if (!hit) {
    hit = lru;
    if (hit == pend.list) { if (int r = flushHeld(false)) return r; }   // slots that still wait are listed in the entry about to be rewritten
    // the pinned copy may still be the source of an in-flight upload, the device copy the argument of a running build: drain before rewriting
    HIPCHK(hipStreamSynchronize(buildStream()));
    if (build_stream) HIPCHK(hipStreamSynchronize(stream));
    if (B > hit->cap) {
      if (hit->d) { HIPCHK(hipFree(hit->d)); HIPCHK(hipHostFree(hit->h)); hit->d = nullptr; hit->h = nullptr; }
      hit->cap = B > 64 ? B : 64;
      HIPCHK(hipMalloc((void**)&hit->d, sizeof(int) * hit->cap)); HIPCHK(hipHostMalloc((void**)&hit->h, sizeof(int) * hit->cap, hipHostMallocDefault));
    }
    memcpy(hit->h, list, sizeof(int) * B); hit->n = B;
    HIPCHK(hipMemcpyAsync(hit->d, hit->h, sizeof(int) * B, hipMemcpyHostToDevice, buildStream()));
  }
  hit->used = ++slot_clock; cur = hit;
  return 0;
}
int FrameSlots::defer_locked(int B, const int* list, const float* base, size_t stride) {
  std::lock_guard<std::mutex> pl(pend_mu);
  if (int r = supersedeHeld(B, list, true, false)) return r;   // (the table kernel rewrites the device marks of every slot it names)
  if (int r = flushHeld(false)) return r;
  const unsigned int gen = build_gen + 1u; build_gen += 3u;
  hipLaunchKernelGGL(dmv::k_attach_deferred, dim3((B + 255) / 256), dim3(256), 0, stream, base, stride, fs, (const int*)cur->d, B, gen);
  pend.base = base; pend.stride = stride; pend.list = cur; pend.flush_gen = gen + 2u;
  int n = 0;
  for (int i = 0; i < B; i++) { if (!slots[list[i]].waiting) n++; slots[list[i]].waiting = i + 1; }
  n_waiting.store(n, std::memory_order_release);
  commit_locked(B, list, base, stride, false);
  HIPCHK(hipGetLastError());
  return 0;
}
#endif
