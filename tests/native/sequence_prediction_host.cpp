// Host build of the rule by which so_icp_register_sequence predicts the next scan's guess (reg_plan.h: predicted_guess) and of the
// window rule it has to satisfy (cube_stable), for the CPU suite (tests/test_sequence_prediction_host.py drives it through ctypes;
// built on demand by the test, g++ -O2 -ffp-contract=off like the library).
#include "reg_plan.h"

using namespace soicp;
using namespace soicp::host;

extern "C" {

void sq_predicted_guess(const double exact[7], const double delta[7], double pred[7]) { predicted_guess(exact, delta, pred); }
void sq_pose_compose(const double a[7], const double d[7], double o[7]) { pose_compose(a, d, o); }
int sq_cube_stable(const int origin[3], const int dims[3], const double t[3], double margin) { return cube_stable(origin, dims, t, margin) ? 1 : 0; }

}  // extern "C"
