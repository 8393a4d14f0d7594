// Host build of the function the export kernel of so_icp_correspondence_geometry calls (superodom_amd/csrc/plane_fit.h:
// plane_fit5_geometry) beside plane_fit5, which the fit pass calls, for tests/test_correspondence_geometry_host.py (ctypes).
// Built on demand by the test with the flags of tests/test_plane_fit_host.py (g++ -O2 -ffp-contract=off).
#include "plane_fit.h"

using namespace soicp;

// plane_fit5_geometry over n correspondences: status, nd[4], coeff, obs[3] and ev[3], nrm[3], mean_abs
extern "C" void cg_fit_geometry(const float* nb, const double* pw, const double* pose7, float sq_max_dist_f, double max_point_dist, int n,
                                double* nd, double* coeff, int* status, int* obs, double* ev, double* nrm, double* mean_abs) {
  const ObsAxes ax = obs_axes(pose_from_array(pose7));
  for (int i = 0; i < n; ++i) {
    double o[4] = {0, 0, 0, 0}, c = 0, e[3] = {0, 0, 0}, v[3] = {0, 0, 0}, m = 0;
    int ob[3] = {-1, -1, -1};
    status[i] = plane_fit5_geometry(nb + 15 * (size_t)i, pw + 3 * (size_t)i, ax, sq_max_dist_f, max_point_dist, o, c, ob, e, v, m);
    for (int k = 0; k < 4; ++k) nd[4 * (size_t)i + k] = o[k];
    coeff[i] = c; mean_abs[i] = m;
    for (int k = 0; k < 3; ++k) { obs[3 * (size_t)i + k] = ob[k]; ev[3 * (size_t)i + k] = e[k]; nrm[3 * (size_t)i + k] = v[k]; }
  }
}

// plane_fit5 on the same inputs
extern "C" void cg_fit_plain(const float* nb, const double* pw, const double* pose7, float sq_max_dist_f, double max_point_dist, int n,
                             double* nd, double* coeff, int* status, int* obs) {
  const ObsAxes ax = obs_axes(pose_from_array(pose7));
  for (int i = 0; i < n; ++i) {
    double o[4] = {0, 0, 0, 0}, c = 0;
    int ob[3] = {-1, -1, -1};
    status[i] = plane_fit5(nb + 15 * (size_t)i, pw + 3 * (size_t)i, ax, sq_max_dist_f, max_point_dist, o, c, ob);
    for (int k = 0; k < 4; ++k) nd[4 * (size_t)i + k] = o[k];
    coeff[i] = c;
    for (int k = 0; k < 3; ++k) obs[3 * (size_t)i + k] = ob[k];
  }
}
