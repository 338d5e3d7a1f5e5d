// RCCL as the library sees it: bound at RUN time by capi_comm.hip, on the first call that needs a communicator.  libdmvio_hip.so itself has no link dependency on librccl.so,
// so hosts without RCCL (a single-GPU workstation, a CPU-only build box) load the library and run everything but the multi-GPU entry points, which then fail with a message
// instead of a loader error.
#pragma once
#include <rccl/rccl.h>   // types and prototypes only
#include <string>
#include "internal.h"

struct RcclApi {
  decltype(&ncclAllReduce) allReduce = nullptr;
  decltype(&ncclAllGather) allGather = nullptr;
  decltype(&ncclCommCount) commCount = nullptr;
  decltype(&ncclCommUserRank) commUserRank = nullptr;
  decltype(&ncclGetUniqueId) getUniqueId = nullptr;
  decltype(&ncclCommInitRank) commInitRank = nullptr;
  decltype(&ncclCommDestroy) commDestroy = nullptr;
  decltype(&ncclGetErrorString) getErrorString = nullptr;
  bool ok = false;
  std::string why;
};
RcclApi& rccl();
#define RCCL_READY() do { if (!rccl().ok) return failmsg("RCCL is not available: " + rccl().why); } while (0)
#define NCCLCHK(x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) return failmsg((std::string("RCCL: ") + rccl().getErrorString(r_) + " in " #x).c_str()); } while (0)
