// Host build of what so_icp_set_sequence_priors adds to the device-free headers, for the CPU suite (tests/test_sequence_priors_host.py
// drives it through ctypes; built on demand by the test, g++ -O2 -ffp-contract=off like the library):
//   reg_plan.h    sequence_solve_kernel: which persistent-solve kernel the launches of a frame of the chained path use
//   pose_prior.h  the forms that take T_meas apart from the prior's other words (pose_prior_add_at) beside the one that does not
#include "pose_prior.h"
#include "reg_plan.h"

using namespace soicp;
using namespace soicp::host;

extern "C" {

int sp_sequence_solve_kernel(int mode, int chained) { return (int)sequence_solve_kernel(mode, chained != 0); }
void sp_solve_kernel_kinds(int out[3]) { out[0] = kSolvePlain; out[1] = kSolvePrior; out[2] = kSolvePriorAtGuess; }
int sp_sums_words() { return (int)(sizeof(LmSums) / sizeof(double)); }
// sums: the words of an LmSums (so_icp_sums), added to in place
void sp_prior_add(const double* P, const double pose[7], double* sums) { pose_prior_add(P, pose, *reinterpret_cast<LmSums*>(sums)); }
void sp_prior_add_at(const double* Tm, const double* P, const double pose[7], double* sums) { pose_prior_add_at(Tm, P, pose, *reinterpret_cast<LmSums*>(sums)); }

}  // extern "C"
