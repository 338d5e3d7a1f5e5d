// The device-resident LM of one alignment problem: the body of k_track_lm and of k_track_lm_w (tracker_kernels.hpp), which include this text.  In scope at the point of
// inclusion: T, TL, TABLE (compile-time), BUILT_CLEAN (-1, compile-time: the slot's stamps say whether the frame is clean; 0 / 1: the verdict of the including kernel's own
// pyramid build, k_track_lm_build), trk (the reference: the kernel argument itself, or k_track_lm_w's copy in LDS), fs, in, out, coarsestLvl, cl.
// Included rather than called: behind a function boundary (forced inline, by reference or by value) the compiler no longer hoists the loads of the kernel-argument reference
// the way it does inside the kernel, and every k_track_lm instantiation comes out with another schedule and register allocation (tools/isa_diff.py: all five differ by
// 20-80 instructions).  Included, four of the five are the same instruction for instruction as before the body was shared; k_track_lm<256, 4, true> differs in two address
// computations (9177 -> 9175 instructions) as soon as k_track_lm_w<256, 4, true> is instantiated in the same unit — listed and measured in profiles/track_multi.md.
  __shared__ float s_stage[(T / 64) * SJ_WAVE_FLOATS];
  __shared__ float s_partH[(T / 64) * 256];
  __shared__ float s_partS[T / 64][8];
  __shared__ float s_tot[ACC_PAD];
  __shared__ EvalP s_e;
  __shared__ double s_H[64], s_b[8], s_x[8];
  __shared__ int s_go, s_trk[8];
  __shared__ LMState S;  // written by lane 0 of wave 0 only
  // the division by the cluster size runs on the vector unit: back to scalar registers, so that what is indexed by the problem or the rank (out, cl.part, cl.log) is addressed
  // from scalar registers and not from per-lane copies that would be spilled across the evaluation loops
  const int prob = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / cl.C)), rank = __builtin_amdgcn_readfirstlane((int)(blockIdx.x % cl.C));
  // `in` is pinned host memory: one read of the 120-byte record per workgroup, kept in LDS
  __shared__ LMProblemIn s_in;
  static_assert(sizeof(LMProblemIn) % 4 == 0 && sizeof(LMProblemIn) <= 256, "LMProblemIn is copied as dwords by one wavefront");
  if (threadIdx.x < sizeof(LMProblemIn) / 4) reinterpret_cast<unsigned int*>(&s_in)[threadIdx.x] = reinterpret_cast<const unsigned int*>(in + prob)[threadIdx.x];
  __syncthreads();
  const LMProblemIn& pin = s_in;
  LMProblemOut& pout = rank == 0 ? out[prob] : *cl.discard;   // `out` is pinned host memory (written once, never read); non-leading workgroups write into device scratch
  unsigned int phase = 0;
  if (threadIdx.x == 0) {
    S.cur = poseFrom7(pin.pose7);
    S.affA = pin.aff[0]; S.affB = pin.aff[1];
    for (int i = 0; i < 5; i++) S.lastRes[i] = __builtin_nan("");
    for (int i = 0; i < 3; i++) S.flow[i] = 1000;
    S.lvl = coarsestLvl; S.st = LM_LEVEL_BEGIN; S.totalIts = 0; S.nEvals = 0; S.nPointEvals = 0; S.haveRepeated = 0;
    S.iteration = 0; S.lambda = 0.01f; S.cutoffRepeat = 1; S.incNorm = 0;
    S.resOnly = 0; S.hStale = 0; S.nResEvals = 0; S.nResPointEvals = 0;
    pout.repeated_lvl = -1; pout.first_pass_res = __builtin_nan("");
  }
  if (threadIdx.x < 64) { s_H[threadIdx.x] = 0; if (threadIdx.x < 8) { s_b[threadIdx.x] = 0; s_x[threadIdx.x] = 0; } }
  initStage<T>(s_stage);
  const int slot = __builtin_amdgcn_readfirstlane(pin.new_slot);   // read from LDS, so a vector register to the compiler: what is addressed by the slot (its planes, its stamps) stays scalar
  // every pixel of the new frame finite (stamped by its pyramid build): the evaluation loop without the isfinite guards gives the same values
  const bool clean = BUILT_CLEAN >= 0 ? BUILT_CLEAN != 0 : __builtin_amdgcn_readfirstlane((int)(fs.bad_gen[slot] != fs.build_gen[slot])) != 0;
  const bool tiled0 = TL && __builtin_amdgcn_readfirstlane((int)fs.tiled0[slot]) != 0;
  long long tStep = 0, tEval = 0;
  unsigned int phase_log = 0;
  for (;;) {
    const long long t0 = wall_clock64();
    if (threadIdx.x < 64) {
      // the control step is ONE dependent chain of ~1100 instructions on this wavefront while its three siblings wait: raised issue priority lets it through ahead of the
      // evaluation waves of the other workgroups that share the SIMD (they lose nothing they could not issue a few cycles later)
      __builtin_amdgcn_s_setprio(3);
      const bool go = lmWaveStep<true>(S, trk, pin, pout, s_tot, s_H, s_b, s_x, s_trk, s_e, threadIdx.x, cl.res_only != 0);
      __builtin_amdgcn_s_setprio(0);
      if (threadIdx.x == 0) s_go = go ? 1 : 0;
    }
    __syncthreads();
    const long long t1 = wall_clock64();
    tStep += t1 - t0;
    if (cl.log && rank == 0 && threadIdx.x == 0) {   // diagnostics: the schedule of evaluations this problem runs (k_track_replay runs it again without the control steps)
      const int k = (int)phase_log;
      int lp = prob;
      asm volatile("" : "+s"(lp));   // the two addresses are formed here (epilogueSlot())
      if (s_go && k < LM_LOG_EVALS) cl.log[(size_t)lp * LM_LOG_EVALS + k] = s_e;
      if (!s_go) cl.log_n[lp] = k < LM_LOG_EVALS ? k : LM_LOG_EVALS;
    }
    phase_log++;
    if (!s_go) break;
    const int lvl = s_e.lvl;
    // the plane's address is wave-uniform (level 0 comes out of the pointer table): keep it in scalar registers
    const float* img = dmvUniformGlobal(fs.level(slot, lvl));
    const int first = rank * T + epilogueSlot();   // this thread's first template record; formed in every round (epilogueSlot())
    if (__builtin_amdgcn_readfirstlane(s_e.res_only)) {   // workgroup-uniform; above level 0 only (lmWaveStep)
      if (clean) blockEvalRes<T, false>(s_e, trk.g[lvl], refPtr<TABLE>(trk.pc[lvl]), refInt<TABLE>(trk.pc_n[lvl]), first, cl.C * T, img, trk.huberTH, s_partS, s_tot);
      else blockEvalRes<T, true>(s_e, trk.g[lvl], refPtr<TABLE>(trk.pc[lvl]), refInt<TABLE>(trk.pc_n[lvl]), first, cl.C * T, img, trk.huberTH, s_partS, s_tot);
    } else if (TL && tiled0 && lvl == 0) {   // workgroup-uniform
      if (clean)
        blockEval<T, false, TL>(s_e, trk.g[lvl], refPtr<TABLE>(trk.pc[lvl]), refInt<TABLE>(trk.pc_n[lvl]), refPtr<TABLE>(trk.flow_mask), first, cl.C * T, img, trk.huberTH, s_stage, s_partH, s_partS,
                                s_tot);
      else
        blockEval<T, true, TL>(s_e, trk.g[lvl], refPtr<TABLE>(trk.pc[lvl]), refInt<TABLE>(trk.pc_n[lvl]), refPtr<TABLE>(trk.flow_mask), first, cl.C * T, img, trk.huberTH, s_stage, s_partH, s_partS,
                               s_tot);
    } else if (clean)
      blockEval<T, false>(s_e, trk.g[lvl], refPtr<TABLE>(trk.pc[lvl]), refInt<TABLE>(trk.pc_n[lvl]), refPtr<TABLE>(trk.flow_mask), first, cl.C * T, img, trk.huberTH, s_stage, s_partH, s_partS,
                          s_tot);
    else
      blockEval<T, true>(s_e, trk.g[lvl], refPtr<TABLE>(trk.pc[lvl]), refInt<TABLE>(trk.pc_n[lvl]), refPtr<TABLE>(trk.flow_mask), first, cl.C * T, img, trk.huberTH, s_stage, s_partH, s_partS,
                         s_tot);
    if (cl.C > 1) { clusterExchange(s_tot, cl, prob, rank, phase); phase++; }
    tEval += wall_clock64() - t1;
  }
  if (threadIdx.x == 0) {
    for (int i = 0; i < 5; i++) pout.lastRes[i] = S.lastRes[i];
    for (int i = 0; i < 3; i++) pout.flow[i] = S.flow[i];
    pout.iterations = S.totalIts;
    pout.n_evals = S.nEvals;
    pout.n_point_evals = S.nPointEvals;
    pout.ticks_step = tStep;
    pout.ticks_eval = tEval;
    pout.n_res_evals = S.nResEvals;
    pout.n_res_point_evals = S.nResPointEvals;
  }
  if (rank == 0) {
    if (threadIdx.x < 64) pout.H[threadIdx.x] = s_H[threadIdx.x];
    if (threadIdx.x < 8) pout.b[threadIdx.x] = s_b[threadIdx.x];
  }
