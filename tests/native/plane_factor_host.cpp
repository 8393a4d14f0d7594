// Host build of superodom_amd/csrc/plane_factor.h (the arithmetic of one plane correspondence is host + device code) for the CPU
// suite: tests/plane_factor_host.py drives it through ctypes.  Built on demand (g++ -O2 -ffp-contract=off).
#include "plane_factor.h"

using namespace soicp;

// n correspondences (p float [3n], normal [3n], d, coeff) at pose7 under TukeyLoss(a2, variant): per point the residual, the weight
// and the cost term; sums29 = the 29 sums added in index order from zero
extern "C" void pfac_evaluate(const float* p, const double* normal, const double* d, const double* coeff, int n, const double* pose7, double a2,
                              int variant, double* residual, double* weight, double* cost_term, double* sums29) {
  const Pose pose = pose_from_array(pose7);
  double R[9];
  quat_to_matrix(pose.q, R);
  const TukeyLoss L(a2, variant);
  for (int k = 0; k < kPlaneFactorSums; ++k) sums29[k] = 0;
  for (int i = 0; i < n; ++i) {
    const double px = (double)p[3 * (size_t)i], py = (double)p[3 * (size_t)i + 1], pz = (double)p[3 * (size_t)i + 2];
    const double* nn = normal + 3 * (size_t)i;
    const double r = plane_residual_at(pose.q, pose.t, px, py, pz, nn[0], nn[1], nn[2], d[i]);
    double rho0, rho1;
    tukey_rho(L, r * r, rho0, rho1);
    residual[i] = r; weight[i] = coeff[i] * rho1; cost_term[i] = 0.5 * coeff[i] * rho0;
    plane_factor_add(R, px, py, pz, nn[0], nn[1], nn[2], coeff[i], r, rho0, weight[i], sums29);
  }
}
