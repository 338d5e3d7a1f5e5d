// The host-driven Gauss-Newton loop of the window optimiser: linearisation, accumulation (+ the three passes of a graph with residuals kept linearised), the energy terms,
// one iteration as named stages (GnIteration), FullSystem::optimize around it and the chain measurement of dmvio_hip_ba_profile_chain.  A declaration file of capi_ba.hip's
// translation unit: included there, once, behind the handle's helpers (fillWindow, dynFromHost, uploadWindowTables, uploadAdjoints, uploadThresholds, makeDecide, waitTicket,
// resolveTh) and ba_shard_host.hpp.  The ORDER of every enqueue, upload, host callback and ticket increment in here is the loop's behaviour.
#pragma once
// ---- linearisation: what varies between the loop's launches of k_ba_linearize (the wide pair / back-substitution structs are cut down to the instantiation's: BA_BY_MAXF)
struct LinearizeArgs {
  const BAWindow* window;          // calibration and frame slots of the state to linearise (the handle's, or the backed-up state's after a rejected step)
  float* fullJ;                    // where the 74-float RawResidualJacobians go, or null
  const unsigned char* mask;       // per point: relinearise only these (marginalisation), or null
  BADecide decide;                 // what the kernel's last workgroup sums and decides
  bool use_backup;                 // restore the points from their backup first (rejected step)
  const BAPreDyn* dyn; bool use_dyn;       // step-dependent pair terms as a kernel argument instead of the device table's
  const ResubArgs* resub; bool do_resub;   // back-substitution + point step fused in front
};
// a linearisation of the handle's current state from the device table, without mask, backup or fused back-substitution
static LinearizeArgs linearizeArgs(dmvio_hip_ba* b, const BADecide& D) {
  return LinearizeArgs{&b->W, b->keep_fullJ ? b->d_fullJ : (float*)nullptr, nullptr, D, false, &b->dyn_cur, false, &b->x_none, false};
}
static void launchLinearize(dmvio_hip_ba* b, const LinearizeArgs& A) {
  b->fullJ_applied = false;
  BA_BY_MAXF(b->H.F, M, hipLaunchKernelGGL((k_ba_linearize<M>), dim3(b->n_lin_blocks), dim3(LIN_THREADS), 0, b->stream, *A.window, b->P, b->Rs, (const BAPrecalc*)b->d_pre,
                                           b->ctx->frames.built_and_waited(), A.fullJ, A.mask, A.decide, (int)BA_GATE_ALWAYS, A.use_backup ? 1 : 0, baNarrow<BAPreDynT<M>>(*A.dyn), A.use_dyn ? 1 : 0,
                                           baNarrow<ResubArgsT<M>>(*A.resub), A.do_resub ? 1 : 0));
}
// FullSystem::linearizeAll (FullSystemOptimize.cpp:150-218) — the energy sum; updates the newest frame's energy threshold (setNewFrameEnergyTH, on the device by the
// kernel's last workgroup) unless TH_KEEP (the caller sets it itself, from energies gathered over shards); fix: + applyRes and linearizeAll(true)'s removal of inactive residuals
enum LinThreshold { TH_UPDATE, TH_KEEP };
static void linearizePickUp(dmvio_hip_ba* b, double* energy, LinThreshold th) {
  *energy = b->h_res->E[0];
  if (th == TH_UPDATE) { b->H.fr[b->H.F - 1].frameEnergyTH = b->h_res->th[0]; b->th_pending = false; }
}
// enqueue only: *ticket is the decision's.  The caller waits for it — or for a LATER ticket of the same stream (kernels it enqueues behind this one) — and then picks the
// results up with linearizePickUp
static int linearizeEnqueue(dmvio_hip_ba* b, bool fix, LinThreshold th, unsigned int* ticket) {
  BAHost& H = b->H;
  if (int r = uploadWindowTables(b)) return r;  // precalc of the current state
  if (int r = uploadThresholds(b)) return r;
  const bool shard = sharded(b);
  if (shard) { if (int r = ensureExchange(b)) return r; }
  // the decision pass (last workgroup of the linearisation) publishes the ticket the host polls; the applyRes kernel of a fix-linearisation runs behind it on the
  // same stream and nothing it writes is read by the host, so no stream synchronisation is needed for it either
  const BADecide D = makeDecide(b, 0, th == TH_UPDATE, true);
  *ticket = D.ticket;
  BA_PROF(b, 0);
  launchLinearize(b, linearizeArgs(b, kernelDecide(b, D)));
  BA_PROF(b, 1);
  if (fix) { hipLaunchKernelGGL(k_ba_apply, dim3((H.R + 255) / 256), dim3(256), 0, b->stream, H.R, b->Rs, (const unsigned char*)nullptr, 1); b->fullJ_applied = b->keep_fullJ; }   // + linearizeAll(true)'s removal of inactive residuals
  HIPCHK(hipGetLastError());
  if (shard) { if (int r = decideGlobal(b, D)) return r; }
  return 0;
}
static int linearizeAll(dmvio_hip_ba* b, bool fix, LinThreshold th, double* energy) {
  unsigned int ticket = 0;
  if (int r = linearizeEnqueue(b, fix, th, &ticket)) return r;
  if (int r = waitTicket(b, ticket)) return r;
  linearizePickUp(b, energy, th);
  return 0;
}
static int applyRes(dmvio_hip_ba* b) {
  hipLaunchKernelGGL(k_ba_apply, dim3((b->H.R + 255) / 256), dim3(256), 0, b->stream, b->H.R, b->Rs, (const unsigned char*)nullptr, 0);
  HIPCHK(hipGetLastError());
  b->fullJ_applied = b->keep_fullJ;
  return 0;
}
// ---- accumulateAF + accumulateSCF + adjoint stitching on the device; result in h_sys = [H_A | b_A | H_sc | b_sc | resInA].  The chains of the host loop are never gated
// (BA_GATE_ALWAYS: gated chains exist only in the device-resident loop, ba_batch_host.hpp) and the host waits for every one of them.
// the gather kernel publishes per workgroup (BAHostRes::gticket): wait until every slot shows the chain's ticket
static int waitGather(dmvio_hip_ba* b, const unsigned int ticket, const int nblk) {
  volatile unsigned int* slots = b->h_res->gticket;
  auto all = [=] { for (int k = nblk - 1; k >= 0; k--) if (slots[k] != ticket) return false; return true; };
  return spinUntil(b, all, "BA kernel chain", "BA accumulation chain finished without publishing its system");
}
// the accumulation + stitching launches over an arbitrary (records, activity, per-point sums) view of the graph
static int accumulateViews(dmvio_hip_ba* b, const BARes& RsV, const BAPoints& PV) {
  BAHost& H = b->H;
  if (b->adj_dirty) { if (int r = uploadAdjoints(b)) return r; }
  const int F = H.F, F2 = F * F, n = H.n(), gate = BA_GATE_ALWAYS;
  hipStream_t s = b->stream;
  AccumArgs A = b->accumArgs();
  const int nblk = b->accBlocks();
  if (b->timing) {
    if (b->accTicksBlocks != nblk) { if (b->d_accTicks) hipFree(b->d_accTicks); HIPCHK(hipMalloc((void**)&b->d_accTicks, sizeof(long long) * 2 * nblk)); b->accTicksBlocks = nblk; }
    A.ticks = b->d_accTicks;
  }
  hipLaunchKernelGGL(k_ba_accumulate, dim3(nblk), dim3(256), 0, s, A, RsV, PV, (const BACtl*)b->d_ctl, gate);
  BA_PROF(b, 3);
  BA_BY_MAXF(F, M, hipLaunchKernelGGL((k_ba_stitch<M>), dim3(F + F2), dim3(64 * F), sizeof(StitchWave) * F, s, F, b->nsTop, b->nsD, b->d_accTop, b->d_numTop, b->d_accD, b->d_numD,
                                      b->d_accE, b->d_adHost, b->d_adTarget, b->SB, (const BACtl*)b->d_ctl, gate));
  BA_PROF(b, 4);
  const int tot = 2 * (n * n + n), n_gather = (tot + 256) / 256;
  if (!sharded(b)) {
    b->acc_ticket = ++b->ticket;
    BA_BY_MAXF(F, M, hipLaunchKernelGGL((k_ba_stitch_gather<M>), dim3(n_gather), dim3(256), 0, s, F, b->nsC, b->d_accC, b->SB, b->d_numTop, F2 * b->nsTop, b->h_sys,
                                        b->d_ctl, gate, b->h_res, b->acc_ticket));
  } else {
    // this rank's part of the system stays in HBM, is summed over the ranks in place and only then published to the host
    BA_BY_MAXF(F, M, hipLaunchKernelGGL((k_ba_stitch_gather<M>), dim3(n_gather), dim3(256), 0, s, F, b->nsC, b->d_accC, b->SB, b->d_numTop, F2 * b->nsTop, b->d_sys,
                                        b->d_ctl, gate, (BAHostRes*)nullptr, 0u));
    HIPCHK(hipGetLastError());
    if (int r = commAllReduceSum(b, b->d_sys, (size_t)tot + 1)) return r;
    b->acc_ticket = ++b->ticket;
    hipLaunchKernelGGL(k_ba_publish_sys, dim3(1), dim3(1024), 0, s, (const double*)b->d_sys, b->h_sys, tot + 1, b->h_res, b->acc_ticket);
  }
  HIPCHK(hipGetLastError());
  BA_PROF(b, 5);
  if (!sharded(b)) { if (int r = waitGather(b, b->acc_ticket, n_gather)) return r; }
  else if (int r = waitTicket(b, b->acc_ticket)) return r;
  H.resInA = (int)b->h_sys[tot];
  return 0;
}
// solveSystemF's three accumulations for a graph with residuals kept linearised (EnergyFunctional.cpp:846-852: accumulateAF_MT, accumulateLF_MT, accumulateSCF_MT).  One
// accumulation kernel serves a (host,target) bucket's top block and its Schur terms from ONE activity flag; here the three reference passes see different sets — addPoint<0>
// the active residuals that are not linearised, addPoint<1> those that are (with the res_toZeroF + J delta record), the Schur side every active one — so the kernel chain
// runs three times over three views and each pass contributes its part: [HL | bL] -> BAHost::HLraw / bLraw, [HA | bA | resInA] and [Hsc | bsc] -> h_sys as always.
static int accumulateLin(dmvio_hip_ba* b, bool backup_points, bool apply_first) {
  BAHost& H = b->H;
  hipStream_t s = b->stream;
  const int R = H.R, N = H.N, n = H.n(), tot = 2 * (n * n + n);
  if (apply_first) { if (int r = applyRes(b)) return r; }
  std::vector<float> adHT;
  H.adHTdeltaF(adHT);   // EnergyFunctional::setDeltaF at the current state
  HIPCHK(b->bounce.h2d(b->d_adHTdelta, adHT.data(), sizeof(float) * adHT.size(), s));
  const float4 cd = make_float4(H.cDeltaF[0], H.cDeltaF[1], H.cDeltaF[2], H.cDeltaF[3]);
  hipLaunchKernelGGL(k_ba_lin_records, dim3((R + 255) / 256), dim3(256), 0, s, b->W, b->P, b->Rs, (const float*)b->d_fullJ, (const unsigned char*)b->d_lin, (const float*)b->d_rtz,
                     (const float*)b->d_adHTdelta, cd, b->d_linRec, b->d_linActive, b->d_topActive);
  hipLaunchKernelGGL(k_ba_lin_point_sums, dim3((N + 255) / 256), dim3(256), 0, s, b->W, b->P, (const float*)b->d_linRec, (const unsigned char*)b->d_linActive, b->d_lHdd, b->d_lbd, b->d_lHcd);
  hipLaunchKernelGGL(k_ba_point_sums, dim3(b->n_pt8_blocks), dim3(256), 0, s, b->W, b->P, b->Rs, backup_points ? 1 : 0, 0, (const BACtl*)b->d_ctl, (int)BA_GATE_ALWAYS,
                     (backup_points && b->vio) ? b->h_idepth_backup : (float*)nullptr);
  HIPCHK(hipGetLastError());
  // L pass
  BARes RsL = b->Rs; RsL.rec[0] = RsL.rec[1] = b->d_linRec; RsL.active = b->d_linActive; RsL.lin = nullptr;
  if (int r = accumulateViews(b, RsL, b->P)) return r;
  H.HLraw.assign(b->h_sys, b->h_sys + (size_t)n * n); H.bLraw.assign(b->h_sys + (size_t)n * n, b->h_sys + (size_t)n * n + n);
  // A pass
  BARes RsA = b->Rs; RsA.active = b->d_topActive;
  if (int r = accumulateViews(b, RsA, b->P)) return r;
  std::vector<double> top(b->h_sys, b->h_sys + (size_t)n * n + n);
  const int resInA = H.resInA;
  // Schur pass
  if (int r = accumulateViews(b, b->Rs, b->P)) return r;
  memcpy(b->h_sys, top.data(), sizeof(double) * top.size());
  b->h_sys[tot] = (double)resInA; H.resInA = resInA;
  return 0;
}
// backup_points: backupState of the points rides in the per-point sums; apply_first: applyRes_Reductor(true) fused into them
static int accumulateWith(dmvio_hip_ba* b, bool backup_points, bool apply_first) {
  if (linAny(b)) return accumulateLin(b, backup_points, apply_first);
  if (apply_first) b->fullJ_applied = b->keep_fullJ;
  hipLaunchKernelGGL(k_ba_point_sums, dim3(b->n_pt8_blocks), dim3(256), 0, b->stream, b->W, b->P, b->Rs, backup_points ? 1 : 0, apply_first ? 1 : 0,
                     (const BACtl*)b->d_ctl, (int)BA_GATE_ALWAYS, (backup_points && b->vio) ? b->h_idepth_backup : (float*)nullptr);
  BA_PROF(b, 2);
  return accumulateViews(b, b->Rs, b->P);
}
static int accumulate(dmvio_hip_ba* b) { return accumulateWith(b, false, false); }                // the system of the state as it stands
static int accumulateBackup(dmvio_hip_ba* b) { return accumulateWith(b, true, false); }           // ... of a state the loop may have to come back to
static int accumulateApplyBackup(dmvio_hip_ba* b) { return accumulateWith(b, true, true); }       // ... of the state the last linearisation evaluated (an accepted step)
// calcLEnergyPt (EnergyFunctional.cpp:349-409) for the residuals kept linearised: (2 res_toZeroF + J delta) . (J delta), summed the way the reference does — an Accumulator11
// (four fp32 lanes; its 1k / 1M levels never fill within a run) per run of 50 points (IndexThreadReduce::reduce with step 50, EnergyFunctional.cpp:427-428), two 4-lane
// updates per residual in point / residual order, the runs' fp32 totals added in double.  The points' own prior term deltaF^2 priorF is zero: idepth_zero follows idepth.
static double linEnergy(dmvio_hip_ba* b) {
  const BAHost& H = b->H;
  std::vector<float> adHT;
  H.adHTdeltaF(adHT);
  double A = 0;
  for (int p0 = 0; p0 < H.N; p0 += 50) {
    float d1[4] = {0, 0, 0, 0};
    for (int pi = p0; pi < std::min(H.N, p0 + 50); pi++)
      for (int ri = b->h_res_begin[pi]; ri < b->h_res_begin[pi + 1]; ri++) {
        if (!b->h_lin[ri] || !b->h_linAct[ri]) continue;
        const float* J = &b->h_linJ[(size_t)ri * FJ_FLOATS];
        const float* rtz = &b->h_rtz[(size_t)ri * 8];
        const float* dp = &adHT[(size_t)(b->h_host[pi] + H.F * b->h_target[ri]) * 8];
        float Jp_delta_x, Jp_delta_y;
        baJpDelta(J, dp, H.cDeltaF, 0.0f, Jp_delta_x, Jp_delta_y);
        for (int i = 0; i < 8; i += 4)
          for (int k = 0; k < 4; k++) d1[k] = d1[k] + baLinEnergyTerm(J, rtz, dp, Jp_delta_x, Jp_delta_y, i + k);
      }
    A += (double)(d1[0] + d1[1] + d1[2] + d1[3]);
  }
  return A;
}
// EnergyFunctional::calcLEnergyF_MT (EnergyFunctional.cpp:414-431)
static double calcLEnergy(dmvio_hip_ba* b) { return b->n_lin > 0 ? b->H.calcLEnergyFrames() + linEnergy(b) : b->H.calcLEnergyFrames(); }
// ... of a window whose points are sharded over ranks: the frame / calibration part is the same on every rank, the linearised residuals' term is this rank's points' share —
// summed over the ranks by one more (one-double) all-reduce, which every rank enters (n_lin_global decides, not the rank's own count)
static int calcLEnergyR(dmvio_hip_ba* b, double* out) {
  if (!sharded(b) || b->n_lin_global == 0) { *out = calcLEnergy(b); return 0; }
  double l = b->n_lin > 0 ? linEnergy(b) : 0.0;
  if (!b->d_red1) { if (dalloc(b, &b->d_red1, 1)) return -1; }
  HIPCHK(b->bounce.h2d(b->d_red1, &l, sizeof(double), b->stream));
  if (int r = commAllReduceSum(b, b->d_red1, 1)) return r;
  HIPCHK(b->bounce.d2h(&l, b->d_red1, sizeof(double), b->stream));
  HIPCHK(b->bounce.finish(b->stream));
  *out = b->H.calcLEnergyFrames() + l;
  return 0;
}
// ---- the reference's default solver branch (setting_useGTSAMIntegration): views of the window for the hooks, calcMEnergyF with the GTSAM term
static void fillFrameViews(dmvio_hip_ba* b) {
  const BAHost& H = b->H;
  b->vio_frames.resize(H.F);
  for (int f = 0; f < H.F; f++) {
    dmvio_hip_ba_frame_view& v = b->vio_frames[f];
    const BAFrameHost& fr = H.fr[f];
    v.frameID = fr.frameID; v.index = f;
    poseTo7(fr.w2c, v.PRE_worldToCam7); poseTo7(fr.evalPT, v.worldToCam_evalPT7);
    memcpy(v.state10, fr.state, sizeof(v.state10)); memcpy(v.state_zero10, fr.state_zero, sizeof(v.state_zero10));
  }
}
// EnergyFunctional::calcMEnergyF (EnergyFunctional.cpp:322-345): without hooks delta.dot(2 bM + HM delta); with them updateBAValues(frames) when the current values are
// asked for, then getBAEnergy(useNewValues) + delta.dot(2 bMForGTSAM + HMForGTSAM delta)
static double calcMEnergy(dmvio_hip_ba* b, bool useNewValues) {
  if (!b->vio) return b->H.calcMEnergy();
  if (!useNewValues && b->vio->updateBAValues) { fillFrameViews(b); b->vio->updateBAValues(b->vio->user, b->H.F, b->vio_frames.data(), b->H.c_value); }
  const double g = b->vio->getBAEnergy ? b->vio->getBAEnergy(b->vio->user, useNewValues ? 1 : 0) : 0.0;
  return g + b->H.calcMEnergy();
}
static double vioDynamicWeight(dmvio_hip_ba* b, double E0, int resInA) {
  if (!b->vio || !b->vio->updateDynamicWeight) return 1.0;
  const float rmse = sqrtf((float)(E0 / (8 * resInA)));   // patternNum * ef->resInA (FullSystemOptimize.cpp:495-498)
  return b->vio->updateDynamicWeight(b->vio->user, E0, (double)rmse, b->vio_opt ? b->vio_opt->coarseTrackingWasGood : 1);
}
// ---- back-substitution and the point step as calls of their own (dmvio_hip_ba_solve, the sharded building blocks); the loop fuses both into its linearisation
static ResubArgs makeResubArgs(BAHost& H, const std::vector<double>& x) {
  ResubArgs X;
  std::vector<float> xAd;
  H.prepareResubstitute(x, X.xc, xAd);
  memset(X.xAd, 0, sizeof(X.xAd));
  memcpy(X.xAd, xAd.data(), sizeof(float) * xAd.size());
  return X;
}
static int resubstitute(dmvio_hip_ba* b, const std::vector<double>& x) {
  const ResubArgs X = makeResubArgs(b->H, x);
  BA_BY_MAXF(b->H.F, M, hipLaunchKernelGGL((k_ba_resubstitute<M>), dim3(b->n_pt8_blocks), dim3(256), 0, b->stream, b->W, b->P, b->Rs, baNarrow<ResubArgsT<M>>(X), 0));
  HIPCHK(hipGetLastError());
  return 0;
}
// mode 0 backup, 1 step from backup, 2 restore; the step-norm sums (mode 1) are only fetched when the caller asks for them
static int pointStep(dmvio_hip_ba* b, int mode, float fac, float* sumID = nullptr, float* sumNID = nullptr) {
  hipLaunchKernelGGL(k_ba_point_step, dim3(b->n_pt_blocks), dim3(256), 0, b->stream, b->H.N, b->P, mode, fac, (mode == 1 && sumID && sumNID) ? b->d_spart : (float*)nullptr);
  HIPCHK(hipGetLastError());
  if (mode == 1 && sumID && sumNID) {
    HIPCHK(hipMemcpyAsync(b->h_spart, b->d_spart, sizeof(float) * 2 * b->n_pt_blocks, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    float a = 0, d = 0;
    for (int i = 0; i < b->n_pt_blocks; i++) { a += b->h_spart[2 * i]; d += b->h_spart[2 * i + 1]; }
    *sumID = a / b->H.N; *sumNID = d / b->H.N;
  }
  return 0;
}
// the energy / threshold of a relinearisation the host did not wait for, once a later ticket of the same stream has been seen (or after waiting for its own)
static int settleReject(dmvio_hip_ba* b, double lastE[3], bool wait) {
  if (!b->pending_reject) return 0;
  if (wait) { if (int r = waitTicket(b, b->pending_ticket)) return r; }
  lastE[0] = b->h_res->E[1];
  b->H.fr[b->H.F - 1].frameEnergyTH = b->h_res->th[1]; b->th_pending = false;
  if (b->pending_trace >= 0 && b->pending_trace < 64) b->trace[b->pending_trace][0] = lastE[0];
  b->pending_reject = false; b->pending_trace = -1;
  return 0;
}
// defer: after a rejected step return without waiting for the relinearisation of the restored state (its energy stays on the device for the next accept test,
// BACtl::lastE0); lastE[0] is then filled in by the next call's wait or by settleReject, and so is row trace_slot of the handle's trace.
// last: the caller will not iterate again — an accepted step is applied, but the system of the new state (which only the next solve would read) is not accumulated: the
// per-point sums (HdiF, idepth_hessian) and resInA then stay those of the last solveSystemF, as in the reference.
struct GnOpts { bool defer = false; int trace_slot = -1; bool last = false; };
struct GnResult {
  int rc = 0;   // 0, or the error the library reported
  bool accepted = false, canbreak = false;   // canbreak: doStepFromBackup's return value && baIntegration->canBreak() (FullSystemOptimize.cpp:520-523); false without hooks
};
// ---- One Gauss-Newton iteration = the loop body of FullSystem::optimize (FullSystemOptimize.cpp:485-586).
// The host solves the 68x68 system (the hand-off point of the reference's GTSAM branch, EnergyFunctional.cpp:958-969) and steps the
// frames; everything else is ONE chain of kernels enqueued without waiting in between:
//   resubstitute + point step  ->  linearise the stepped state, its last workgroup sums the energy, sets the newest keyframe's threshold
//   and takes the accept / reject decision  ->  [rejected only] restore the points and relinearise the backed-up state  ->  [accepted only]
//   applyRes + per-point sums + point backup -> accumulation -> adjoint stitching -> the stitched system of the NEW state in host memory.
// The host waits once per iteration, by polling the ticket the chain's last kernel stores behind its results.  After a rejected step the
// system in host memory is still the one of the (restored) state, so the next iteration reuses the system at hand and goes straight to its solve with the larger lambda.
// Its stages, in the order run() calls them, and what one stage leaves for a later one:
struct GnIteration {
  dmvio_hip_ba* const b; BAHost& H;
  const int iteration; double& lambda;
  double* const lastE;   // [3]: photometric, linearised + prior, marginalisation (+ GTSAM) energy of the state at hand
  const GnOpts opt;
  const int n, tot; const bool shard, dynDuring; const dmvio_hip_ba_callbacks* const vio;
  bool last;
  double tq0 = 0, tq1 = 0;
  std::vector<double> x;                      // solve -> step
  BAWindow W_backup; BAPreDyn dyn_backup;     // step -> rejected: calibration (W) and step-dependent precalc members of the backed-up state
  ResubArgs X;                                // step -> decide
  double newL = 0, newM = 0;                  // step -> decide, accepted
  unsigned int D_ticket = 0;                  // decide -> accepted
  GnResult res;
  GnIteration(dmvio_hip_ba* b_, int iteration_, double& lambda_, double lastE_[3], const GnOpts& opt_)
      : b(b_), H(b_->H), iteration(iteration_), lambda(lambda_), lastE(lastE_), opt(opt_), n(b_->H.n()), tot(2 * (n * n + n)), shard(sharded(b_)),
        dynDuring(b_->vio && b_->vio_opt && b_->vio_opt->updateDynamicWeightDuringOptimization), vio(b_->vio), last(opt_.last) {}
#define BA_PH(i) do { if (b->timing) { tq1 = nowUs(); b->tm.t[i] += tq1 - tq0; tq0 = tq1; } } while (0)
  // backupState (the point part rode in the per-point sums that produced the system at hand), and that system unless the previous iteration left it behind
  int systemAtHand() {
    H.backupFrames();
    H.prepareSolve();   // nullspaces, orthogonalisation basis, prior right-hand side
    if (!b->sys_ready) { if (int r = accumulateBackup(b)) return r; }
    b->sys_ready = false;
    return 0;
  }
  // the weight of the photometric energy against the GTSAM factors, updated before solving (FullSystemOptimize.cpp:491-503); ef->resInA is the count the LAST
  // solveSystemF left behind — before the first solve of this call the caller's (vio_options::resInA_at_entry) or, without one, the current system's
  int dynamicWeight() {
    if (!(vio && (dynDuring || iteration == 0))) return 0;
    if (b->pending_reject) { if (int r = settleReject(b, lastE, true)) return r; }
    const int resInA_ref = iteration == 0 ? ((b->vio_opt && b->vio_opt->resInA_at_entry >= 0) ? b->vio_opt->resInA_at_entry : (int)b->h_sys[tot]) : b->resInA_solve;
    b->dynW = vioDynamicWeight(b, lastE[0], resInA_ref);
    return 0;
  }
  // solveSystem: the library's own damped LDLT, or the caller's solver
  int solve() {
    const double* p = b->h_sys;
    b->resInA_solve = (int)p[tot];
    if (!vio) { H.solveSystem(iteration, lambda, p, p + n * n, p + n * n + n, p + 2 * n * n + n, x); return 0; }
    // hand-over of EnergyFunctional.cpp:958-969: the damped Schur system, its right-hand side and the undamped system go to the caller's solver
    std::vector<double> HP((size_t)n * n), bP(n), HN((size_t)n * n);
    H.buildGtsamSystem(lambda, p, p + n * n, p + n * n + n, p + 2 * n * n + n, HP.data(), bP.data(), HN.data());
    fillFrameViews(b);
    x.assign(n, 0.0);
    if (!vio->computeBAUpdate) return failmsg("ba_optimize_vio: computeBAUpdate hook missing");
    if (vio->computeBAUpdate(vio->user, n, HP.data(), bP.data(), lambda, HN.data(), H.F, b->vio_frames.data(), H.c_value, x.data()) != 0)
      return failmsg("ba_optimize_vio: computeBAUpdate hook reported an error");
    H.finishExternalSolve(iteration, x);
    return 0;
  }
  // doStepFromBackup, frames and calibration (resubstituteF_MT + the point part, stepfac 1, ride in front of the linearisation of the stepped state), its canbreak test,
  // and the host's energy terms of the stepped state
  int stepAndCanbreak() {
    X = makeResubArgs(H, x);
    // the step norms only feed canbreak, which stays false without the GTSAM hooks (FullSystemOptimize.cpp:387,523,583)
    if (!b->pre_static_valid) { if (int r = uploadWindowTables(b)) return r; }   // evaluation-point members of the table (R0, t0, b0): once per window
    fillWindow(b);
    dynFromHost(H, b->dyn_cur);         // backed-up state, for a relinearisation after a rejected step
    W_backup = b->W;
    dyn_backup = b->dyn_cur;
    float fs[4];
    H.stepFrames(1.0f, fs);
    H.setPrecalcValues();
    if (vio) {
      // FullSystemOptimize.cpp:269-313: sumNID = mean |idepth_backup| over the points in window order (the per-point sums mirrored idepth_backup into host memory)
      float sumNID = 0, numID = 0;
      for (int pi = 0; pi < H.N; pi++) { sumNID += fabsf(b->h_idepth_backup[pi]); numID++; }
      sumNID /= numID;
      const float thOpt = H.S.thOptIterations;
      res.canbreak = sqrtf(fs[0]) < 0.0005 * thOpt && sqrtf(fs[1]) < 0.00005 * thOpt && sqrtf(fs[3]) < 0.00005 * thOpt && sqrtf(fs[2]) * sumNID < 0.00005 * thOpt;
      res.canbreak = res.canbreak && vio->canBreak && vio->canBreak(vio->user) != 0;
    }
    const int minOpt = (b->vio_opt && b->vio_opt->minOptIterations >= 0) ? b->vio_opt->minOptIterations : H.S.minOptIterations;
    if (res.canbreak && iteration >= minOpt) last = true;
    if (int r = calcLEnergyR(b, &newL)) return r;
    newM = calcMEnergy(b, true);
    if (dynDuring) b->dynW = vioDynamicWeight(b, lastE[0], b->resInA_solve);   // before deciding whether to accept the step (FullSystemOptimize.cpp:534-538)
    return 0;
  }
  // linearise the stepped state; the kernel's last workgroup sums the energy, sets the newest keyframe's threshold and decides; wait for the decision
  int decide() {
    fillWindow(b);
    dynFromHost(H, b->dyn_cur);
    if (int r = uploadThresholds(b)) return r;
    BA_PH(2);
    BADecide D = makeDecide(b, 1, true, true);
    D_ticket = D.ticket;
    // newEnergy[0] + newEnergy[1] + newEnergyL + newEnergyM / dynamicGTSAMWeight (FullSystemOptimize.cpp:553-554): the quotients are formed here (x / 1.0 == x without hooks)
    D.lastE0 = lastE[0]; D.lastL = lastE[1]; D.lastM = lastE[2] / b->dynW; D.newL = newL; D.newM = newM / b->dynW;
    D.lastE0_from_ctl = b->pending_reject ? 1 : 0;   // the host has not seen the restored state's energy yet: the device has
    LinearizeArgs A = linearizeArgs(b, kernelDecide(b, D));
    A.use_dyn = true; A.resub = &X; A.do_resub = true;
    launchLinearize(b, A);
    HIPCHK(hipGetLastError());
    if (shard) { if (int r = decideGlobal(b, D)) return r; }
    BA_PH(3);
    if (int r = waitTicket(b, D.ticket)) return r;   // energy and the accept / reject decision are in host memory (the threshold follows: resolveTh)
    if (int r = settleReject(b, lastE, false)) return r;   // ... and so are those of an earlier relinearisation on the same stream
    BA_PH(4);
    res.accepted = b->h_res->accept != 0;
    return 0;
  }
  // applyRes + per-point sums + point backup -> accumulation -> stitching: the system of the new state, for the next iteration's solve.
  // (Enqueuing this branch speculatively behind the linearisation, gated on the device-side decision, was measured: no gain — the four
  // launches, not the host round trip, set its length.)
  int accepted() {
    if (!last) { if (int r = accumulateApplyBackup(b)) return r; }
    else { if (int r = applyRes(b)) return r; }
    lastE[0] = b->h_res->E[0]; lastE[1] = newL; lastE[2] = newM;
    b->th_pending = true; b->th_pending_ticket = D_ticket;   // the threshold follows its decision by a few microseconds: picked up by resolveTh before anything reads it
    lambda = std::max(lambda * 0.25, 1e-5);
    if (vio && vio->acceptBAUpdate) vio->acceptBAUpdate(vio->user, lastE[0]);   // FullSystemOptimize.cpp:569-572
    return 0;
  }
  // loadSateBackup + linearizeAll (FullSystemOptimize.cpp:575-581): the points are restored by the relinearisation kernel itself; the
  // system in host memory is still the one of the restored state
  int rejected() {
    const BADecide D2 = makeDecide(b, 2, true, true);
    LinearizeArgs A = linearizeArgs(b, kernelDecide(b, D2));
    A.window = &W_backup; A.use_backup = true; A.dyn = &dyn_backup; A.use_dyn = true;
    launchLinearize(b, A);
    HIPCHK(hipGetLastError());
    if (shard) { if (int r = decideGlobal(b, D2)) return r; }
    H.restoreFrames();
    H.setPrecalcValues();
    fillWindow(b);
    b->dyn_cur = dyn_backup;
    if (int r = calcLEnergyR(b, &lastE[1])) return r;
    lastE[2] = calcMEnergy(b, false);
    b->pending_reject = true; b->pending_ticket = D2.ticket; b->pending_trace = opt.trace_slot;
    if (!opt.defer) { if (int r = settleReject(b, lastE, true)) return r; }
    lambda *= 1e2;
    return 0;
  }
  int run() {
    if (shard) { if (int r = ensureExchange(b)) return r; }
    tq0 = b->timing ? nowUs() : 0;
    if (int r = systemAtHand()) return r;
    if (int r = dynamicWeight()) return r;
    BA_PH(0);
    if (int r = solve()) return r;
    BA_PH(1);
    if (int r = stepAndCanbreak()) return r;
    if (int r = decide()) return r;
    if (int r = res.accepted ? accepted() : rejected()) return r;
    BA_PH(5);
    b->sys_ready = !(res.accepted && last);   // accepted: the chain left the system of the new state behind; rejected: the one at hand still is the restored state's
    b->tm.n++;
    return 0;
  }
#undef BA_PH
};
static GnResult gnIteration(dmvio_hip_ba* b, int iteration, double& lambda, double lastE[3], const GnOpts& opt) {
  GnIteration it(b, iteration, lambda, lastE, opt); it.res.rc = it.run(); return it.res;
}
// FullSystem::optimize (FullSystemOptimize.cpp:417-647).  vio == NULL: the library's own damped LDLT (the reference's solver with setting_useGTSAMIntegration off);
// otherwise every solve, the M-energy term, the dynamic weight and the early exit go through the caller's hooks, in the order the reference calls BAGTSAMIntegration.
static int optimizeImpl(dmvio_hip_ba* b, int mnumOptIts, const dmvio_hip_ba_callbacks* vio, const dmvio_hip_ba_vio_options* opt, float* rmse, double* finalEnergy, int* iterations,
                        double* trace /* 64x4 or NULL */) {
  BAHost& H = b->H;
  if (H.F < 2) { if (rmse) *rmse = 0; return 0; }
  mnumOptIts = BAHost::optIterations(H.F, mnumOptIts);
  struct VioScope {   // the hooks are those of this call only
    dmvio_hip_ba* b;
    ~VioScope() { b->vio = nullptr; b->vio_opt = nullptr; b->H.gtsam = false; b->dynW = 1.0; }
  } scope{b};
  b->vio = vio; b->vio_opt = vio ? opt : nullptr; b->dynW = 1.0;
  const int n = H.n();
  if (vio) {
    H.gtsam = true;
    if (opt && opt->HMForGTSAM && opt->bMForGTSAM) { H.HMG.assign(opt->HMForGTSAM, opt->HMForGTSAM + (size_t)n * n); H.bMG.assign(opt->bMForGTSAM, opt->bMForGTSAM + n); }
    else { H.HMG.assign((size_t)n * n, 0.0); H.bMG.assign(n, 0.0); }
  }
  if (int r = dmvio_hip_ba_activate_all(b)) return r;
  double lastE[3];
  // initial linearisation, applyRes and the first system (per-point sums → accumulation → stitching) go out as ONE chain: nothing in it waits for the host, which
  // picks the energy and the threshold up behind the chain's last ticket
  unsigned int lin_ticket = 0;
  if (int r = linearizeEnqueue(b, false, TH_UPDATE, &lin_ticket)) return r;
  if (int r = applyRes(b)) return r;
  if (int r = accumulateBackup(b)) return r;   // backupState of the points rides in the per-point sums; the frames are backed up by the first iteration
  linearizePickUp(b, &lastE[0], TH_UPDATE);
  b->sys_ready = true;
  if (int r = calcLEnergyR(b, &lastE[1])) return r;
  lastE[2] = calcMEnergy(b, false);
  double lambda = 1e-5;
  int done = 0;
  b->trace[0][0] = lastE[0]; b->trace[0][1] = lastE[1]; b->trace[0][2] = lastE[2]; b->trace[0][3] = 1;
  for (int iteration = 0; iteration < mnumOptIts; iteration++) {
    GnOpts o;
    o.defer = true; o.trace_slot = done + 1; o.last = iteration == mnumOptIts - 1;
    const GnResult g = gnIteration(b, iteration, lambda, lastE, o);
    if (g.rc) return g.rc;
    done++;
    if (done < 64) { b->trace[done][0] = lastE[0]; b->trace[done][1] = lastE[1]; b->trace[done][2] = lastE[2]; b->trace[done][3] = g.accepted ? 1 : 0; }
    // canbreak && iteration >= setting_minOptIterations (FullSystemOptimize.cpp:586): baIntegration->canBreak() stays false without the GTSAM hooks
    const int minOpt = (opt && vio && opt->minOptIterations >= 0) ? opt->minOptIterations : H.S.minOptIterations;
    if (g.canbreak && iteration >= minOpt) break;
  }
  if (int r = settleReject(b, lastE, true)) return r;
  if (vio) b->dynW = vioDynamicWeight(b, lastE[0], b->resInA_solve);   // "Update again!" (FullSystemOptimize.cpp:594)
  // fix the newest frame's linearisation point, re-linearise with applyRes (FullSystemOptimize.cpp:596-609)
  H.reanchorNewest();
  if (int r = uploadAdjoints(b)) return r;   // (nothing is enqueued between the two: the upload stands in the stream where it stood inside the sequence)
  double fe = 0;
  if (int r = linearizeAll(b, true, TH_UPDATE, &fe)) return r;
  b->final_energy = fe; b->iterations_done = done;
  if (rmse) *rmse = sqrtf((float)(fe / (8 * H.resInA)));
  if (finalEnergy) *finalEnergy = fe;
  if (iterations) *iterations = done;
  if (trace) memcpy(trace, b->trace, sizeof(b->trace));
  if (vio && vio->postOptimization) { fillFrameViews(b); vio->postOptimization(vio->user, H.F, b->vio_frames.data(), H.c_value); }   // FullSystemOptimize.cpp:641
  return 0;
}
// Measurement (dmvio_hip_ba_profile_chain): the kernel chain of an ACCEPTED Gauss-Newton iteration on the current state — linearise (+ energy / threshold decision pass) ->
// applyRes + per-point sums -> accumulate -> adjoint stitch -> gather — `reps` times, with HIP events recorded on the handle's stream between the launches; us5 = mean
// microseconds of the five kernels (each figure includes the gap to the next launch: what the chain costs on the stream).  The window state is left as a linearise +
// applyRes + accumulate leaves it.
static int profileChain(dmvio_hip_ba* b, int reps, float us5[5]) {
  struct Events {   // destroyed on every way out
    hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (int k = 0; k < 6; k++) if (e[k]) hipEventDestroy(e[k]); }
  } evs;
  hipEvent_t* ev = evs.e;
  for (int k = 0; k < 6; k++) HIPCHK(hipEventCreate(&ev[k]));
  struct ProfScope { dmvio_hip_ba* b; ~ProfScope() { b->prof = nullptr; } } profScope{b};
  double acc[5] = {0, 0, 0, 0, 0};
  int rc = 0;
  for (int r = 0; r < reps && rc == 0; r++) {
    unsigned int ticket = 0;
    b->prof = ev;
    rc = linearizeEnqueue(b, false, TH_UPDATE, &ticket);
    if (rc == 0) rc = accumulateApplyBackup(b);
    b->prof = nullptr;
    HIPCHK(hipStreamSynchronize(b->stream));
    for (int k = 0; k < 5; k++) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, ev[k], ev[k + 1])); acc[k] += 1e3 * ms; }
  }
  for (int k = 0; k < 5; k++) us5[k] = (float)(acc[k] / reps);
  return rc;
}
