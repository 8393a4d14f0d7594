// Host build of superodom_amd/csrc/plane_fit.h (the product's plane fit is host + device code) for the CPU suite:
// tests/test_plane_fit_host.py drives it through ctypes.  Built on demand by the test (g++ -O2 -ffp-contract=off).
#include "plane_fit.h"

using namespace soicp;

// fit(nb, pw, axes, nd, coeff, obs) -> status, over n correspondences
template <typename Fit>
static void fit_all(Fit fit, const float* nb, const double* pw, const double* pose7, int n, double* nd /*4n*/, double* coeff /*n*/,
                    int* status /*n*/, int* obs /*3n*/) {
  const Pose pose = pose_from_array(pose7);
  const ObsAxes ax = obs_axes(pose);
  for (int i = 0; i < n; ++i) {
    double o[4] = {0, 0, 0, 0}, c = 0;
    int ob[3] = {-1, -1, -1};
    status[i] = fit(nb + 15 * (size_t)i, pw + 3 * (size_t)i, ax, o, c, ob);
    for (int k = 0; k < 4; ++k) nd[4 * (size_t)i + k] = o[k];
    coeff[i] = c;
    for (int k = 0; k < 3; ++k) obs[3 * (size_t)i + k] = ob[k];
  }
}

// plane_fit5: the closed form (production)
extern "C" void pf_fit(const float* nb, const double* pw, const double* pose7, float sq_max_dist_f, double max_point_dist, int n,
                       int obs_as_written, double* nd, double* coeff, int* status, int* obs) {
  fit_all([=](const float* b, const double* w, const ObsAxes& ax, double* o, double& c, int* ob) {
    return plane_fit5(b, w, ax, sq_max_dist_f, max_point_dist, o, c, ob, obs_as_written != 0);
  }, nb, pw, pose7, n, nd, coeff, status, obs);
}

// plane_fit5_reference: column-pivoted Householder plane, with jacobi_eig the cyclic Jacobi eigen-solver (the flag comes LAST: this
// entry has no obs_as_written)
extern "C" void pf_fit_reference(const float* nb, const double* pw, const double* pose7, float sq_max_dist_f, double max_point_dist, int n,
                                 double* nd, double* coeff, int* status, int* obs, int jacobi_eig) {
  fit_all([=](const float* b, const double* w, const ObsAxes& ax, double* o, double& c, int* ob) {
    return plane_fit5_reference(b, w, ax, sq_max_dist_f, max_point_dist, o, c, ob, jacobi_eig != 0);
  }, nb, pw, pose7, n, nd, coeff, status, obs);
}
