// Host build of what so_icp_set_batch_priors adds to the device-free headers, for the CPU suite (tests/test_batch_priors_host.py drives
// it through ctypes; built on demand by the test, g++ -O2 -ffp-contract=off like the library):
//   reg_plan.h    batch_solve_kernel: which batched solve kernel a round of so_icp_register_batch launches for its active list
#include "reg_plan.h"

using namespace soicp::host;

extern "C" {

// modes: SO_ICP_PRIOR_* per hypothesis of the group (NULL: the batch carries no priors); active: the round's list
int bp_batch_solve_kernel(const uint8_t* modes, const uint32_t* active, uint32_t n_active) { return (int)batch_solve_kernel(modes, active, n_active); }
void bp_batch_solve_kernel_kinds(int out[2]) { out[0] = kBatchSolvePlain; out[1] = kBatchSolvePrior; }

}  // extern "C"
