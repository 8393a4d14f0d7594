// solve_kernel_body.inc -- the body of solve_kernel, solve_kernel_prior, solve_kernel_prior_at_guess and solve_kernel_batch_prior
// (kernels.hip), included once for each with
//   SO_BODY_KERNEL  the kernel's own instantiation (its kernarg lines)
//   SO_BODY_PRIOR   0 / 1 / kPriorAtGuess / kPriorBatch: eval_pass without the pose prior / with it / with it, T_meas = DevState::pose_in /
//                   with the prior of the workgroup's hypothesis, where that has one
//   SO_BODY_PRIOR_WORDS   nullptr / the prior's 55 doubles (the kernel's last argument) / prior_block
//   SO_BODY_PRIOR_TABLE   (solve_kernel_batch_prior only) the table of per-hypothesis prior blocks, the kernel's last argument
// and PROF, BATCH, PEER in scope.  One text, four kernels of different names: a registration or a batch without a prior launches the
// functions it always launched.
  __shared__ EvalShared sh;
  __shared__ CorrCache cache;  // 26 KB next to the 64 KB of EvalShared: gfx950 has 160 KB of LDS per CU, one workgroup each here
  // The non-batched launch's image of the state block up to `seq` (4 KB; workgroup 0 alone fills and uses it): loaded here, in the
  // shadow of the fit pass; a solve that ends writes its results into it and the block goes out once (eval_pass, flush_state_image).
  constexpr bool kStateImage = SO_ENDGAME_IMAGE != 0 && !BATCH;
  __shared__ u4v state_image[kStateImage ? kStateChunks + 1 : 1];
  DevState* const img = reinterpret_cast<DevState*>(state_image);
  unsigned long long t_entry = 0;
  if (PROF && !BATCH) t_entry = wall_clock64();  // (profiling: "kernel entry -> first pass begins", word 3 of the fit record)
  if (SO_ENTRY_WARM) st = after_loaded(st, kernarg_lines<decltype(&SO_BODY_KERNEL)>());
  WgSpan span{0, 0, 0, false};
#ifdef SO_BODY_PRIOR_TABLE
  const double* prior_block = nullptr;  // this workgroup's hypothesis' block of the prior table
#endif
  if (BATCH) {
    const uint32_t G = bv.wg_per_hyp, hi = blockIdx.x / G, sub = blockIdx.x - hi * G;
    const size_t h = bv.active[hi];
#ifdef SO_BODY_PRIOR_TABLE
    prior_block = SO_BODY_PRIOR_TABLE + h * kBatchPriorStride;
#endif
    st += h; corr.nd += h * bv.bs; corr.coeff += h * bv.bs; corr.status += h * bv.bs; nbr5 += h * 5 * bv.bs;
    partials += h * bv.partial_stride; ticket += h * bv.sync_stride; hist += h * (kHistReplicas * kHistStride);
    span.V = bv.v_grid;
    span.vb0 = (uint32_t)(((unsigned long long)sub * bv.v_grid) / G);
    span.vb1 = (uint32_t)(((unsigned long long)(sub + 1u) * bv.v_grid) / G);
    span.ctl = sub == 0;
  }
  if (SO_ENTRY_WARM) st = after_loaded(st, state_lines<true, !BATCH>(st));
  if (st->reg_done) return;
  if (!BATCH && ep.chain_expect && st->done_count != ep.chain_expect) return;  // chained registration whose predecessor was not over: no-op
  const int tid = threadIdx.x;
  // kPriorAtGuess: the measurement is the guess this registration's BEGIN launch stored (reg_begin_state) -- an earlier launch of
  // the same queue, so a plain load; once, by the controller's first wavefront, the only one that reads it (eval_pass:
  // prior_prepare_at, in front of the polling loop of every pass).  Behind the two returns above: a launch enqueued behind the
  // registration's converged iteration, or behind a registration in front that was not over, never gets here, and a launch that
  // does runs before the BEGIN launch of the next registration, which is behind it in the queue and the only writer of pose_in.
  [[maybe_unused]] double prior_tm[7] = {0, 0, 0, 0, 0, 0, 1};
  if constexpr (SO_BODY_PRIOR == kPriorAtGuess) {
    if (blockIdx.x == 0 && tid < 64) {
#pragma unroll
      for (int i = 0; i < 7; ++i) prior_tm[i] = st->pose_in[i];
    }
  }
  // hand-off record: 8 chunks of 16 bytes {value, epoch}, each written / read with ONE sc1 dwordx4 access (atomic as a
  // unit), so a reader that sees the expected epoch in a chunk has that chunk's value: no second round trip, no
  // publisher-side wait between data and flag.  Chunks 0..6 = next pose, chunk 7 = "another evaluation follows".
  u4v* hand = reinterpret_cast<u4v*>(ticket + kHandoffWordOffset);
  // epoch base of this launch: a kernel argument (the host counts its solve launches; 32 epochs per launch), larger than
  // every epoch an earlier launch left in the hand-off record -- no memory round trip before the first pass can start
  const unsigned long long e0 = ep.epoch_base;
  Pose pose = pose_from_array(st->T);
  if (tid == 0) {  // the controller's inputs are constant over the launch (read here, next to the pose: no fetch inside a pass)
    sh.peer_seq = st->peer_seq;
    for (int i = 0; i < 3; ++i) sh.ctl.T[i] = pose.t[i];
    for (int i = 0; i < 4; ++i) sh.ctl.T[3 + i] = pose.q[i];
    sh.ctl.lm_max = st->lm_max; sh.ctl.outer_iter = st->outer_iter; sh.ctl.max_outer = st->max_outer;
  }
  const unsigned long long tag0 = (e0 + 1ull) << 5;  // pass tags: unique over launches (every launch advances the epoch) and passes (slot <= 16)
  if (kStateImage && blockIdx.x == 0) {  // (nothing else writes *st while this launch runs: its kernels are one queue's, in order)
    const u4v* block = reinterpret_cast<const u4v*>(st);
    for (int i = tid; i < kStateChunks; i += 256) state_image[i] = block[i];
  }
  if (PROF && !BATCH && (ep.ablate & 128) && blockIdx.x == 0) {
    if (kStateImage) __syncthreads();  // (the stamp's word has been loaded)
    if (tid == 0) (kStateImage ? img : st)->dbg[3] = wall_clock64() - t_entry;
  }
  int code = eval_pass<true, true, PROF, BATCH, PEER, SO_BODY_PRIOR>(0, 1, pose, spx, spy, spz, corr, st, ep, partials, ticket, hist, out, mpts, nbr5, mp, sh, SO_BODY_PRIOR_WORDS, tag0, &cache, hand, e0 + 1ull, span, prior_tm, img);
  for (int slot = 1; slot <= lm_max; ++slot) {
    __syncthreads();
    const unsigned long long want = e0 + (unsigned long long)slot;
    if (code == kPassMore || code == kPassDone) {
      // this workgroup ran the controller, whose thread has already published {request, more?} with epoch `want` and
      // left them in sh.pose / sh.more
    } else if (tid < 64) {  // wait for the controller's workgroup: lanes 0..7 poll one chunk each
      bool done = tid >= 8;
      unsigned long long val = 0;
      const unsigned long long t0 = wall_clock64();
      bool ok = true;
      for (;;) {
        if (!done) {
          const u4v v = load16_sc1(hand + tid);
          const unsigned long long tag = ((unsigned long long)v.w << 32) | v.z;
          if (tag - e0 >= (unsigned long long)slot && tag - e0 <= 64ull) { done = true; val = ((unsigned long long)v.y << 32) | v.x; }
        }
        if (__ballot(!done) == 0ull) break;
        // (the controller's workgroup may itself be waiting for the other ranks' records: twice its patience + the local 50 ms)
        if (wall_clock64() - t0 > 2ull * ep.timeout_ticks + 5000000ull) { ok = false; break; }  // give up instead of hanging the device
        __builtin_amdgcn_s_sleep(1);
      }
      if (tid < 7) sh.pose[tid] = __longlong_as_double((long long)val);
      if (tid == 7) sh.more = ok ? (int)val : -1;
    }
    __syncthreads();
    if (sh.more != 1) return;  // solve ended (or timeout)
    pose = pose_from_array(sh.pose);
    __syncthreads();
    code = eval_pass<false, true, PROF, BATCH, PEER, SO_BODY_PRIOR>(slot, 1, pose, spx, spy, spz, corr, st, ep, partials, ticket, hist, out, mpts, nbr5, mp, sh, SO_BODY_PRIOR_WORDS, tag0 + (unsigned long long)slot, &cache, hand, want + 1ull, span, prior_tm, img);
  }
