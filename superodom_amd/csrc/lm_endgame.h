// lm_endgame.h -- what the device controller decides about the END of a solve ahead of lm_solver.h's protocol (kernels.hip
// lm_control_wave).  Plain C++ next to lm_solver.h: the kernels and the host tests (tests/test_solve_endgame_host.py) compile this text.
#pragma once
#include <cmath>

#include "lm_solver.h"

namespace soicp {

// ParameterToleranceReached is the first test of lm_feed and reads nothing of the candidate's sums: step_norm = |x - cand| and x_norm
// are known when the candidate is proposed.  `sn` is the square lm_after_candidate forms (same FMA chain, same bits), so
// sqrt(sn) below IS the step_norm the next lm_feed would compare: true exactly when that lm_feed ends with termination 2, whatever
// sums it is fed (NaN in either operand: false on both sides).
// The first line is the cheap side: thr^2 (1 + 1e-7) < sn puts the correctly rounded root above thr by 4e-8 thr, far more than the
// two roundings of the product can move it (thr >= 1e-16: no underflow; thr^2 = inf or NaN: not taken) -- one product and one
// comparison on the common path, the square root only for a step of about the tolerance's size.
SO_HD bool lm_parameter_tolerance_at_proposal(double sn, double x_norm) {
  const double thr = LmConst::kParameterTolerance * (x_norm + LmConst::kParameterTolerance);
  if (sn > thr * thr * 1.0000001) return false;
  return sqrt(sn) <= thr;
}

}  // namespace soicp
