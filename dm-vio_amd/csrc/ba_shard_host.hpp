// Exchange steps of the sharded Gauss-Newton iteration (dmvio_hip_ba_set_comm / _set_comm_callbacks): every rank holds all keyframes and ITS points.  With an RCCL
// communicator the exchanges are enqueued on the handle's stream between the kernels that produce and consume the buffers (no host hop); the callback transport stages
// them through host memory.  A declaration file of capi_ba.hip's translation unit: included there, once, behind the handle (ba_handle.h), dalloc and makeDecide.
#pragma once

static bool sharded(const dmvio_hip_ba* b) { return b->world > 0; }
static bool linAny(const dmvio_hip_ba* b) { return sharded(b) ? b->n_lin_global > 0 : b->n_lin > 0; }   // any rank holds a residual kept linearised
static hipEvent_t* commEvents(dmvio_hip_ba* b, const int kind) {
  b->comm_total[kind]++;
  if (!b->comm_timing || b->comm_n[kind] >= dmvio_hip_ba::COMM_EVS) return nullptr;
  hipEvent_t* e = b->comm_ev[kind][b->comm_n[kind]];
  if (!e[0] && (hipEventCreate(&e[0]) != hipSuccess || hipEventCreate(&e[1]) != hipSuccess)) return nullptr;
  b->comm_n[kind]++;
  return e;
}
static int commAllReduceSum(dmvio_hip_ba* b, double* d_buf, size_t count) {
  if (b->nccl) {
    hipEvent_t* e = commEvents(b, 0);
    if (e) HIPCHK(hipEventRecord(e[0], b->stream));
    NCCLCHK(rccl().allReduce(d_buf, d_buf, count, ncclDouble, ncclSum, b->nccl, b->stream));
    if (e) HIPCHK(hipEventRecord(e[1], b->stream));
    return 0;
  }
  b->h_stage.resize(count);
  HIPCHK(hipMemcpyAsync(b->h_stage.data(), d_buf, sizeof(double) * count, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (b->comm_cb.allreduce_sum_f64(b->comm_cb.user, b->h_stage.data(), count) != 0) return failmsg("comm callback allreduce_sum_f64 failed");
  HIPCHK(hipMemcpyAsync(d_buf, b->h_stage.data(), sizeof(double) * count, hipMemcpyHostToDevice, b->stream));
  return 0;
}
static int commAllGather(dmvio_hip_ba* b, const float* d_in, float* d_out, size_t count_per_rank) {
  if (b->nccl) {
    hipEvent_t* e = commEvents(b, 1);
    if (e) HIPCHK(hipEventRecord(e[0], b->stream));
    NCCLCHK(rccl().allGather(d_in, d_out, count_per_rank, ncclFloat, b->nccl, b->stream));
    if (e) HIPCHK(hipEventRecord(e[1], b->stream));
    return 0;
  }
  const size_t bytes = sizeof(float) * count_per_rank;
  b->h_stage.resize((bytes * (b->world + 1) + 7) / 8);
  char* in = (char*)b->h_stage.data(); char* out = in + bytes;
  HIPCHK(hipMemcpyAsync(in, d_in, bytes, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (b->comm_cb.allgather(b->comm_cb.user, in, out, bytes) != 0) return failmsg("comm callback allgather failed");
  HIPCHK(hipMemcpyAsync(d_out, out, bytes * b->world, hipMemcpyHostToDevice, b->stream));
  return 0;
}
// record width of the decision exchange: agreed on once per graph (the largest per-rank number of residuals that target the newest keyframe)
static int ensureExchange(dmvio_hip_ba* b) {
  if (b->xchg_width) return 0;
  int mine = (int)b->h_newest.size(), widest = mine;
  if (b->world > 1) {
    float* d_tmp = nullptr;
    if (dalloc(b, &d_tmp, (size_t)b->world + 1)) return -1;
    const float v = (float)mine;   // exact below 2^24 residuals
    HIPCHK(hipMemcpyAsync(d_tmp, &v, sizeof(float), hipMemcpyHostToDevice, b->stream));
    if (int r = commAllGather(b, d_tmp, d_tmp + 1, 1)) return r;
    std::vector<float> all(b->world);
    HIPCHK(hipMemcpyAsync(all.data(), d_tmp + 1, sizeof(float) * b->world, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (float a : all) widest = std::max(widest, (int)a);
  }
  b->xchg_width = BA_XCHG_HEADER + ((widest + 1) & ~1);   // even: the fp64 energy of every record stays 8-byte aligned
  if (dalloc(b, &b->d_xchg_local, (size_t)b->xchg_width) || dalloc(b, &b->d_xchg_all, (size_t)b->xchg_width * b->world)) return -1;
  return 0;
}
// tail of a sharded linearisation: the linearisation's last workgroup packed this rank's record (mode 3); gather the records of all ranks and take
// the decisions of `D` over their union
static int decideGlobal(dmvio_hip_ba* b, BADecide D) {
  if (int r = commAllGather(b, b->d_xchg_local, b->d_xchg_all, (size_t)b->xchg_width)) return r;
  D.xchg_all = b->d_xchg_all; D.xchg_width = b->xchg_width; D.world = b->world;
  hipLaunchKernelGGL(k_ba_decide_global, dim3(1), dim3(256), 0, b->stream, D);
  HIPCHK(hipGetLastError());
  return 0;
}
// the linearisation kernel's view of a decision block when the points are sharded: pack only
static BADecide packOnly(dmvio_hip_ba* b, const BADecide& D) {
  BADecide Dp = D;
  Dp.mode = 3; Dp.publish = 0; Dp.xchg_local = b->d_xchg_local; Dp.xchg_width = b->xchg_width;
  return Dp;
}
// ... of a decision the loop takes: the kernel's last workgroup takes it itself on a single device, and leaves it to decideGlobal on a sharded window
static BADecide kernelDecide(dmvio_hip_ba* b, const BADecide& D) { return sharded(b) ? packOnly(b, D) : D; }
