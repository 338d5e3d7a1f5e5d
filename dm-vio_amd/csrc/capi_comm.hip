// libdmvio_hip.so — the RCCL run-time loader and the communicator entry points (include/dmvio_hip.h, "multi-GPU").  No kernels: the collectives of the sharded BA
// iteration are enqueued by capi_ba.hip through rccl_api.h, the tracker's hypothesis exchange is set up here.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <memory>
#include <mutex>
#include <string>

#include "../../include/dmvio_hip.h"
#include "tracker_handle.h"
#include "rccl_api.h"

RcclApi& rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    void* h = nullptr;
    for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) { h = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) { api.why = std::string("librccl.so cannot be loaded (") + (dlerror() ? dlerror() : "?") + ")"; return; }
    bool all = true;
    auto get = [&](const char* sym) { void* p = dlsym(h, sym); if (!p) { all = false; api.why = std::string("librccl.so lacks ") + sym; } return p; };
    api.allReduce = (decltype(api.allReduce))get("ncclAllReduce"); api.allGather = (decltype(api.allGather))get("ncclAllGather");
    api.commCount = (decltype(api.commCount))get("ncclCommCount"); api.commUserRank = (decltype(api.commUserRank))get("ncclCommUserRank");
    api.getUniqueId = (decltype(api.getUniqueId))get("ncclGetUniqueId"); api.commInitRank = (decltype(api.commInitRank))get("ncclCommInitRank");
    api.commDestroy = (decltype(api.commDestroy))get("ncclCommDestroy"); api.getErrorString = (decltype(api.getErrorString))get("ncclGetErrorString");
    api.ok = all;
  });
  return api;
}

// hypothesis-parallel trackNewCoarse: the element-wise fp64 sum over all ranks of a small HOST buffer, in place; dmvio_hip_tracker_track_new_coarse
// (capi.hip) calls it
static int dmv_tracker_set_exchange(dmvio_hip_tracker* t, std::function<int(double*, size_t)> allreduce_sum, int rank, int world) {
  if (!t) return failmsg("null tracker");
  // dmvio_hip_tracker_debug_split_single_rank(t, 1) (tests): a group of ONE rank still takes the split path — every try is "mine", the all-reduce is the identity — so
  // that the exchange (RCCL on the context's stream included) runs on a one-device box.  An explicit call on THIS tracker, never the environment.
  const bool force1 = world == 1 && allreduce_sum && t->debug_split1;
  if ((world <= 1 && !force1) || !allreduce_sum) { t->xchg = nullptr; t->xrank = 0; t->xworld = 0; return 0; }
  if (rank < 0 || rank >= world) return failmsg("tracker_set_comm: 0 <= rank < world");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  t->xchg = std::move(allreduce_sum); t->xrank = rank; t->xworld = world;
  return 0;
}

extern "C" {
int dmvio_hip_comm_unique_id(unsigned char id128[128]) {
  if (!id128) return failmsg("null argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  RCCL_READY();
  ncclUniqueId id;
  NCCLCHK(rccl().getUniqueId(&id));
  memcpy(id128, &id, 128);
  return 0;
}
int dmvio_hip_comm_init_rank(dmvio_hip_ctx* ctx, const unsigned char id128[128], int rank, int world, void** out) {
  if (!ctx || !id128 || !out) return failmsg("null argument");
  HIPCHK(hipSetDevice(ctx->device));
  RCCL_READY();
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  ncclComm_t comm = nullptr;
  NCCLCHK(rccl().commInitRank(&comm, world, id, rank));
  *out = (void*)comm;
  return 0;
}
// ---- hypothesis-parallel FullSystem::trackNewCoarse (include/dmvio_hip.h): the per-try records of dmvio_hip_tracker_track_new_coarse summed over the ranks
int dmvio_hip_tracker_set_comm(dmvio_hip_tracker* t, void* nccl_comm, int rank, int world) {
  if (!t) return failmsg("null tracker");
  dmvio_hip_ctx* c = t->ctx;
  const bool force1 = world == 1 && nccl_comm && t->debug_split1;   // test hook (dmvio_hip_tracker_debug_split_single_rank), see dmv_tracker_set_exchange
  if (!nccl_comm || (world <= 1 && !force1)) return dmv_tracker_set_exchange(t, nullptr, 0, 0);
  ncclComm_t comm = (ncclComm_t)nccl_comm;
  RCCL_READY();
  int n = 0, r = -1;
  NCCLCHK(rccl().commCount(comm, &n));
  NCCLCHK(rccl().commUserRank(comm, &r));
  if (n != world || r != rank) return failmsg("tracker_set_comm: rank / world do not match the communicator");
  // 20 doubles per hypothesis: a few KB, staged through a device buffer that stays with the exchange (and through the context's pinned staging area) for RCCL on the context's stream
  struct XchgBuf { double* d = nullptr; size_t cap = 0; int device = 0; ~XchgBuf() { if (d) { hipSetDevice(device); hipFree(d); } } };
  std::shared_ptr<XchgBuf> st = std::make_shared<XchgBuf>();
  st->device = c->device;
  return dmv_tracker_set_exchange(t, [c, comm, st](double* buf, size_t count) -> int {
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    if (count > st->cap) {
      if (st->d) { HIPCHK(hipFree(st->d)); st->d = nullptr; st->cap = 0; }
      HIPCHK(hipMalloc((void**)&st->d, sizeof(double) * 2 * count));
      st->cap = 2 * count;
    }
    HIPCHK(c->bounce.h2d(st->d, buf, sizeof(double) * count, c->stream));
    const ncclResult_t nr = rccl().allReduce(st->d, st->d, count, ncclDouble, ncclSum, comm, c->stream);
    if (nr != ncclSuccess) return failmsg(std::string("RCCL: ") + rccl().getErrorString(nr) + " in the hypothesis exchange");
    HIPCHK(c->bounce.d2h(buf, st->d, sizeof(double) * count, c->stream));
    HIPCHK(c->bounce.finish(c->stream));
    return 0;
  }, rank, world);
}
int dmvio_hip_tracker_set_comm_callbacks(dmvio_hip_tracker* t, const dmvio_hip_comm_callbacks* cb, int rank, int world) {
  if (!t) return failmsg("null tracker");
  if (!cb || world <= 1) return dmv_tracker_set_exchange(t, nullptr, 0, 0);
  if (!cb->allreduce_sum_f64) return failmsg("tracker_set_comm_callbacks: allreduce_sum_f64 is required");
  const dmvio_hip_comm_callbacks k = *cb;
  return dmv_tracker_set_exchange(t, [k](double* buf, size_t count) -> int {
    return k.allreduce_sum_f64(k.user, buf, count) == 0 ? 0 : failmsg("comm callback allreduce_sum_f64 failed");
  }, rank, world);
}
// ncclCommCount / ncclCommUserRank of a communicator: what RCCL itself says about the group (bench.py prints it in the N > 1 line)
int dmvio_hip_comm_info(void* comm, int* n_ranks, int* rank) {
  if (!comm) return failmsg("null communicator");
  RCCL_READY();
  int n = 0, r = -1;
  NCCLCHK(rccl().commCount((ncclComm_t)comm, &n));
  NCCLCHK(rccl().commUserRank((ncclComm_t)comm, &r));
  if (n_ranks) *n_ranks = n;
  if (rank) *rank = r;
  return 0;
}
int dmvio_hip_comm_destroy(void* comm) {
  if (!comm) return 0;
  RCCL_READY();
  NCCLCHK(rccl().commDestroy((ncclComm_t)comm));
  return 0;
}
}  // extern "C"
