// plane_factor.h -- the arithmetic of one accepted plane correspondence (SurfNormAnalyticCostFunction under
// ScaledLoss(TukeyLoss(a), c)), stated once for the evaluation of a registration (kernels.hip eval_pass), the export and the sums of the
// kept set (corr_kernels.hip, corr_sums_kernels.hip) and a host build (tests/native/plane_factor_host.cpp): residual, loss, Jacobian
// row and the 29 sums.  Only + - * / and explicit SO_FMA on plain doubles, compiled with -ffp-contract=off on both sides: every user
// forms the same bits, so a record's residual and weight at the last evaluation's pose are the values that evaluation used.
// (eval_pass takes everything but the loss from here: its Tukey branch is written out there, profiles/plane_factor/README.md says why.)
#pragma once
#include "so_math.h"

namespace soicp {

// the sums of one evaluation: cost, count, Jtr[6], JtJ[21] (upper triangle, row-major) -- the head of LmSums
constexpr int kPlaneFactorSums = 29;

// r = n . w + d at the world point w = R(q) p + t  (lidarOptimization.cpp:61).  Fused: no thresholds downstream, see SO_FMA
SO_HD double plane_residual(double nx, double ny, double nz, double d, double wx, double wy, double wz) {
  return SO_FMA(nx, wx, SO_FMA(ny, wy, SO_FMA(nz, wz, d)));
}
// the same from the sensor-frame point: rotate, translate (lidarOptimization.cpp:59 == LidarSlam.cpp:397-398), residual
SO_HD double plane_residual_at(const double q[4], const double t[3], double px, double py, double pz, double nx, double ny, double nz, double d) {
  double wx, wy, wz;
  quat_rotate<double>(q, px, py, pz, wx, wy, wz);
  wx += t[0]; wy += t[1]; wz += t[2];
  return plane_residual(nx, ny, nz, d, wx, wy, wz);
}

// TukeyLoss(a) [UPSTREAM ceres loss_function.cc], a^2 from LidarSlam.cpp:271: the constants of a pass, formed once.  The quotient s / a^2
// is a product with the reciprocal (the IEEE division sequence is ~28 instructions per correspondence and evaluation); it feeds the
// weights only -- the comparison s <= a^2 is on s itself.  variant 0: rho = a^2/6 (1 - v^3), 1: a^2/3 (1 - v^3), v = 1 - s / a^2.
// (A constructor: returned by value from a function, the constants move correspondences_kernel's listing.)
struct TukeyLoss {
  double a2, inv_a2, rho_out;
  int variant;
  SO_HD TukeyLoss(double a2_, int variant_) : a2(a2_), inv_a2(1.0 / a2_), rho_out((variant_ == 0) ? a2_ / 6.0 : a2_ / 3.0), variant(variant_) {}
};
// rho(s), rho'(s) at s = r^2; rho'' <= 0, so the corrector of ScaledLoss leaves the weight of a correspondence at c rho'
SO_HD void tukey_rho(const TukeyLoss& L, double s, double& rho0, double& rho1) {
  if (s <= L.a2) {
    const double v = 1.0 - s * L.inv_a2, v2 = v * v;
    rho0 = L.rho_out * (1.0 - v2 * v); rho1 = (L.variant == 0) ? 0.5 * v2 : v2;
  } else {
    rho0 = L.rho_out; rho1 = 0;
  }
}

// One correspondence into the 29 sums: J = [n^T, -n^T R [p]x] = [n^T, (p x R^T n)^T] (lidarOptimization.cpp:68-74; R row-major, p the
// SENSOR-frame point), cost += 0.5 c rho, count += 1, Jtr += J w r, JtJ += w J J^T with w = c rho'.
SO_HD void plane_factor_add(const double R[9], double px, double py, double pz, double nx, double ny, double nz, double c, double r, double rho0,
                            double w, double* acc /*kPlaneFactorSums*/) {
  const double m0 = SO_FMA(R[0], nx, SO_FMA(R[3], ny, R[6] * nz));
  const double m1 = SO_FMA(R[1], nx, SO_FMA(R[4], ny, R[7] * nz));
  const double m2 = SO_FMA(R[2], nx, SO_FMA(R[5], ny, R[8] * nz));
  const double J[6] = {nx, ny, nz, SO_FMA(py, m2, -(pz * m1)), SO_FMA(pz, m0, -(px * m2)), SO_FMA(px, m1, -(py * m0))};
  acc[0] = SO_FMA(0.5 * c, rho0, acc[0]);
  acc[1] += 1.0;
  const double wr = w * r;
  int k = 8;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    acc[2 + a] = SO_FMA(J[a], wr, acc[2 + a]);
    const double wj = w * J[a];
#pragma unroll
    for (int b = a; b < 6; ++b) { acc[k] = SO_FMA(wj, J[b], acc[k]); ++k; }
  }
}

}  // namespace soicp
