// corr_sums_body.inc -- the bodies of corr_sums_kernels.hip's kernels, included once for each kernel with
//   SO_SUMS_ADD        0: the per-tile partial sums (correspondence_sums_kernel, selection_correspondence_sums_kernel)
//                      1: the tiles added in tile order (correspondence_sums_add_kernel, selection_correspondence_sums_add_kernel)
//   SO_SUMS_SELECTION  0: one kept set, the kernel's arguments as they are
//                      1: entry blockIdx.y (partial sums) or blockIdx.x / n_poses (add) of a selection of kept sets -- a batch's
//                         hypotheses or a run's frames --, whose point and tile counts may differ (the grid is as wide as the largest
//                         entry; a workgroup beyond its entry's tiles leaves at once): an entry's records, scan and loss come from
//                         its CorrSelEntry, it has n_poses poses and one histogram of its own, and its partial vectors lie at
//                         tile_first[entry] x n_poses, [pose][tile] inside
// One text per pair, two kernels each: so_icp_correspondence_sums launches the functions it always launched, and an entry's sums are
// formed by the same expressions, the same tree and the same tile order as those of a context that kept that entry alone.
#if !SO_SUMS_ADD
  constexpr int kPer = (int)(kCorrTile / 256u), kAcc = (int)kCorrSumsAcc;
  static_assert(kAcc == kPlaneFactorSums, "plane_factor_add fills a partial vector");
  __shared__ SumsPose s_pose[kCorrSumsMaxPoses];
  __shared__ double s_part[2][4][kAcc];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#if SO_SUMS_SELECTION
  const uint32_t entry = blockIdx.y, bid = blockIdx.x;  // (no look-back here, so no ticket: the launch index serves)
  const CorrSelEntry& E = entries[entry];
  const uint32_t n = E.n;
  if (bid * kCorrTile >= n) return;  // (an entry smaller than the largest of the selection; the whole workgroup, in front of every barrier)
  const uint32_t tile0 = tile_first[entry], ntile = tile_first[entry + 1u] - tile0;
  const float* __restrict__ scan = scan_all + (size_t)E.scan_at * 3;
  const double4* __restrict__ cnd = cnd_all + (size_t)E.at;
  const double* __restrict__ ccoeff = ccoeff_all + (size_t)E.at;
  const uint8_t* __restrict__ cstatus = cstatus_all + (size_t)E.at;
  const double a2 = E.a2;
  const int variant = E.variant;
  const double* __restrict__ poses = poses_all + (size_t)entry * n_poses * 7;
  double* __restrict__ partials = partials_all + (size_t)tile0 * n_poses * kAcc;
#define SO_SUMS_NTILE ntile
#else
  const uint32_t bid = blockIdx.x;
#define SO_SUMS_NTILE gridDim.x
#endif
  if ((uint32_t)tid < n_poses) {
    SumsPose P;
    for (int k = 0; k < 3; ++k) P.t[k] = poses[(size_t)tid * 7 + k];
    for (int k = 0; k < 4; ++k) P.q[k] = poses[(size_t)tid * 7 + 3 + k];
    quat_to_matrix(P.q, P.R);
    s_pose[tid] = P;
  }
  const TukeyLoss L(a2, variant);
  bool ok[kPer];
  double pp[kPer][3];
  double4 nd[kPer];
  double co[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const uint32_t i = bid * kCorrTile + (uint32_t)q * 256u + (uint32_t)tid;
    ok[q] = false;
    pp[q][0] = pp[q][1] = pp[q][2] = 0;
    nd[q] = make_double4(0, 0, 0, 0); co[q] = 0;
    if (i < n && cstatus[i] == 0) {  // MatchingResult::SUCCESS
      ok[q] = true;
      pp[q][0] = (double)scan[(size_t)i * 3]; pp[q][1] = (double)scan[(size_t)i * 3 + 1]; pp[q][2] = (double)scan[(size_t)i * 3 + 2];
      nd[q] = cnd[i]; co[q] = ccoeff[i];
    }
  }
  __syncthreads();
  for (uint32_t k = 0; k < n_poses; ++k) {
    const SumsPose& P = s_pose[k];
    double acc[kAcc];
#pragma unroll
    for (int a = 0; a < kAcc; ++a) acc[a] = 0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      if (!ok[q]) continue;
      const double r = plane_residual_at(P.q, P.t, pp[q][0], pp[q][1], pp[q][2], nd[q].x, nd[q].y, nd[q].z, nd[q].w);
      double rho0, rho1;
      tukey_rho(L, r * r, rho0, rho1);
      plane_factor_add(P.R, pp[q][0], pp[q][1], pp[q][2], nd[q].x, nd[q].y, nd[q].z, co[q], r, rho0, co[q] * rho1, acc);
    }
#pragma unroll
    for (int a = 0; a < kAcc; ++a) {
      double v = acc[a];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
      acc[a] = v;
    }
    // (two buffers: the readers of pose k are past the barrier of pose k + 1 before pose k + 2 is written)
    double (*part)[kAcc] = s_part[k & 1u];
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < kAcc; ++a) part[wave][a] = acc[a];
    }
    __syncthreads();
    if (tid < kAcc) partials[((size_t)k * SO_SUMS_NTILE + bid) * kAcc + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
  }
#undef SO_SUMS_NTILE
#else
  constexpr uint32_t kAcc = kCorrSumsAcc, kWords = kCorrSumsWords, kChunk = 64;
  __shared__ double s_in[kChunk * kAcc];
  const uint32_t k = blockIdx.x, tid = threadIdx.x;
#if SO_SUMS_SELECTION
  const uint32_t entry = k / n_poses, tile0 = tile_first[entry], nblk = tile_first[entry + 1u] - tile0;
  const double* mine = partials + ((size_t)tile0 * n_poses + (size_t)(k - entry * n_poses) * nblk) * kAcc;
#else
  const double* mine = partials + (size_t)k * nblk * kAcc;
#endif
  double v = 0;
  for (uint32_t b0 = 0; b0 < nblk; b0 += kChunk) {
    const uint32_t tiles = nblk - b0 < kChunk ? nblk - b0 : kChunk;
    for (uint32_t w = tid; w < tiles * kAcc; w += 256u) s_in[w] = mine[(size_t)b0 * kAcc + w];
    __syncthreads();
    if (tid < kAcc)
      for (uint32_t b = 0; b < tiles; ++b) v += s_in[b * kAcc + tid];
    __syncthreads();
  }
  if (tid < kAcc) sums_out[(size_t)k * kWords + tid] = v;
#if SO_SUMS_SELECTION
  else if (tid < kWords) sums_out[(size_t)k * kWords + tid] = hists[(size_t)(k / n_poses) * (kWords - kAcc) + (tid - kAcc)];
#else
  else if (tid < kWords) sums_out[(size_t)k * kWords + tid] = hist.v[tid - kAcc];
#endif
#endif
