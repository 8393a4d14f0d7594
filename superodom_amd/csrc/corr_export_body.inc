// corr_export_body.inc -- the body of correspondences_kernel and selection_correspondences_kernel (corr_kernels.hip), included once
// for each with
//   SO_CORR_SELECTION  0: one kept set; the ticket is the tile, and scan, cnd, ccoeff, cstatus, n, pose, records, status_out,
//                         residual_out, n_accepted, tile_cost and state are the kernel's arguments
//                      1: a selection of kept sets -- a batch's hypotheses or a run's frames --, whose point and tile counts may
//                         differ: ticket -> (entry, tile) is reg_plan.h's selection_ticket over the prefix table tile_first; the
//                         kernel's arguments are the arrays of ALL entries, and the body offsets to the entry's records, scan and
//                         outputs and takes its loss and pose from its CorrSelEntry before the per-point text (no residual_out: the
//                         records carry the residuals)
// One text, two kernels: the export of a single registration launches the function it always launched.
  constexpr int kPer = (int)(kCorrTile / 256u);
  __shared__ uint32_t s_bid, s_pre[kPer * 4], s_agg, s_excl;
  __shared__ double s_cost[4];
  __shared__ uint2 s_rec[256 * (kCorrRecordBytes / 8)];  // the records of one round, in output order
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_bid = atomicAdd(ticket, 1u);
  __syncthreads();
#if SO_CORR_SELECTION
  // entry-major: the tickets of entry k are tile_first[k] .. tile_first[k + 1] - 1, so a workgroup's look-back waits only for workgroups
  // with smaller tickets, which were handed out earlier and therefore run; the entry's chain starts at its own word 0 of the state
  // table.  An entry without tiles has no ticket (its count stays the zero it was cleared to)
  if (s_bid >= n_tiles) return;  // (never: the launch has n_tiles workgroups)
  const host::BatchTicket mine_of = host::selection_ticket(s_bid, tile_first, n_sel, n_tiles);  // (reg_plan.h)
  const uint32_t entry = mine_of.entry, bid = mine_of.tile;
  const CorrSelEntry& E = entries[entry];
  const uint32_t n = E.n, tile0 = tile_first[entry], nblk = tile_first[entry + 1u] - tile0;
  const float* __restrict__ scan = scan_all + (size_t)E.scan_at * 3;
  const double4* __restrict__ cnd = cnd_all + (size_t)E.at;
  const double* __restrict__ ccoeff = ccoeff_all + (size_t)E.at;
  const uint8_t* __restrict__ cstatus = cstatus_all + (size_t)E.at;
  const Pose pose = pose_from_array(E.pose);
  const double a2 = E.a2;
  const int variant = E.variant;
  uint8_t* __restrict__ records = records_all + (size_t)E.rec_first * kCorrRecordBytes;
  uint8_t* __restrict__ status_out = status_all + (size_t)E.status_first;
  uint32_t* __restrict__ n_accepted = counts + entry;
  double* __restrict__ tile_cost = tile_cost_all + tile0;
  unsigned long long* __restrict__ state = state_all + tile0;
#else
  const uint32_t bid = s_bid;
#endif
  const TukeyLoss L(a2, variant);
  unsigned long long bal[kPer];
  float pf[kPer][3];
  double4 nd[kPer];
  double co[kPer], res[kPer], wgt[kPer];
  double cost = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const uint32_t i = bid * kCorrTile + (uint32_t)q * 256u + (uint32_t)tid;
    bool ok = false;
    pf[q][0] = pf[q][1] = pf[q][2] = 0.0f;
    nd[q] = make_double4(0, 0, 0, 0); co[q] = 0; res[q] = 0; wgt[q] = 0;
    if (i < n) {
      const uint8_t status = cstatus[i];
      ok = status == 0;  // MatchingResult::SUCCESS
#if !SO_CORR_SELECTION
      float rf = __builtin_nanf("");
#endif
      if (ok) {
        pf[q][0] = scan[(size_t)i * 3]; pf[q][1] = scan[(size_t)i * 3 + 1]; pf[q][2] = scan[(size_t)i * 3 + 2];
        nd[q] = cnd[i]; co[q] = ccoeff[i];
        const double r = plane_residual_at(pose.q, pose.t, (double)pf[q][0], (double)pf[q][1], (double)pf[q][2], nd[q].x, nd[q].y, nd[q].z, nd[q].w);
        double rho0, rho1;
        tukey_rho(L, r * r, rho0, rho1);
        res[q] = r; wgt[q] = co[q] * rho1;
        cost = SO_FMA(0.5 * co[q], rho0, cost);
#if !SO_CORR_SELECTION
        rf = (float)r;
#endif
      }
      status_out[i] = status;
#if !SO_CORR_SELECTION
      residual_out[i] = rf;
#endif
    }
    bal[q] = __ballot(ok);
    if (lane == 0) s_pre[q * 4 + wave] = (uint32_t)__popcll(bal[q]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cost += __shfl_xor(cost, d, 64);
  if (lane == 0) s_cost[wave] = cost;
  __syncthreads();
  if (tid == 0) {  // exclusive prefix in scan order: round-major, then wavefront
    uint32_t acc = 0;
    for (int k = 0; k < kPer * 4; ++k) { const uint32_t v = s_pre[k]; s_pre[k] = acc; acc += v; }
    s_agg = acc;
    tile_cost[bid] = ((s_cost[0] + s_cost[1]) + s_cost[2]) + s_cost[3];
  }
  __syncthreads();
  const uint32_t agg = s_agg;
  if (wave == 0) {
    const uint32_t excl = lookback_exclusive(state, bid, agg, lane);
    if (lane == 0) {
      if (bid == nblk - 1u) *n_accepted = excl + agg;
      s_excl = excl;
    }
  }
  __syncthreads();
  const uint32_t excl = s_excl;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const bool mine = (bal[q] >> lane) & 1ull;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[q] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[q], 0u));
    const uint32_t i = bid * kCorrTile + (uint32_t)q * 256u + (uint32_t)tid;
    // The round's records are one contiguous range of the output: laid out in LDS, then stored by the whole workgroup, lane after
    // lane (a lane storing its own 72-byte record, 72 bytes from its neighbour's, measured 0.3 - 1.4 us slower per 131 072-point scan)
    const uint32_t first = s_pre[q * 4], count = (q + 1 < kPer ? s_pre[(q + 1) * 4] : s_agg) - first;
    if (mine) {  // so_icp_correspondence: index, p[3] | n[3] | d | coeff | residual | weight
      uint2* o = s_rec + (size_t)(s_pre[q * 4 + wave] - first + below) * (kCorrRecordBytes / 8);
      double* od = reinterpret_cast<double*>(o);
      o[0] = make_uint2(i, __float_as_uint(pf[q][0]));
      o[1] = make_uint2(__float_as_uint(pf[q][1]), __float_as_uint(pf[q][2]));
      od[2] = nd[q].x; od[3] = nd[q].y; od[4] = nd[q].z; od[5] = nd[q].w;
      od[6] = co[q]; od[7] = res[q]; od[8] = wgt[q];
    }
    __syncthreads();
    uint2* out8 = reinterpret_cast<uint2*>(records + ((size_t)excl + first) * kCorrRecordBytes);
    for (uint32_t w = (uint32_t)tid; w < count * (kCorrRecordBytes / 8); w += 256u) out8[w] = s_rec[w];
    __syncthreads();
  }
