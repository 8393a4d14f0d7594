// Host build of superodom_amd/csrc/reg_plan.h (the decisions of a registration's host schedule that need no device) for the CPU suite:
// tests/test_reg_plan_host.py drives it through ctypes.  Built on demand by the test (g++ -O2).
#include "reg_plan.h"

using namespace soicp::host;

extern "C" {

int rp_outer_limit(int max_iterations) { return outer_limit(max_iterations); }
int rp_lm_limit(int lm_max_iterations) { return lm_limit(lm_max_iterations); }
int rp_outer_cap() { return kOuterCap; }
unsigned long long rp_max_scan_points() { return (unsigned long long)kMaxScanPoints; }
unsigned long long rp_kept_upper_bound(int max_sf, unsigned long long n) { return (unsigned long long)kept_upper_bound(max_sf, (size_t)n); }
int rp_query_wave_count_ok(int max_sf, unsigned long long n, unsigned long long max_kept) { return query_wave_count_ok(max_sf, (size_t)n, (size_t)max_kept) ? 1 : 0; }
// out = {own_full, own_tail, n_own}
void rp_query_split_share(unsigned long long n, unsigned long long world, unsigned long long rank, unsigned long long out[3]) {
  const QueryShare q = query_split_share((size_t)n, (size_t)world, (size_t)rank);
  out[0] = q.own_full; out[1] = q.own_tail ? 1 : 0; out[2] = q.n_own;
}
unsigned rp_bin_table_log2(unsigned long long n) { return bin_table_log2((size_t)n); }
int rp_work_list_fits(unsigned long long bin_packed, unsigned long long wavefronts) { return work_list_fits(bin_packed, wavefronts) ? 1 : 0; }
// out = {kPriorsNone, kPriorSingle, kPriorsRun, kPriorsBatch}
void rp_prior_kinds(int out[4]) { out[0] = kPriorsNone; out[1] = kPriorSingle; out[2] = kPriorsRun; out[3] = kPriorsBatch; }
int rp_refused_prior(int pending, int accepted) { return refused_prior((PriorKind)pending, (PriorKind)accepted); }
int rp_carries_pose_prior(int pending, int own, int world_size, int match_only) { return carries_pose_prior(pending != 0, own != 0, world_size, match_only != 0) ? 1 : 0; }
int rp_cube_stable(const int origin[3], const int dims[3], const double t[3], double margin) { return cube_stable(origin, dims, t, margin) ? 1 : 0; }

}  // extern "C"
