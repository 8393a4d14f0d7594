// pose_prior.cpp -- the absolute pose prior of the reference's Ceres problem (addAbsolutePoseConstraints, LidarSlam.cpp:285-297) inside the
// device solve: so_icp_pose_prior_from_information and so_icp_pose_prior_sums are host arithmetic (pose_prior.h, the header the kernels
// compile too); so_icp_set_pose_prior keeps the prior for the launches of the next registration, whose last argument it becomes;
// so_icp_set_sequence_priors keeps one per frame for the next sequence call (sequence.cpp, localization_sequence.cpp);
// so_icp_set_batch_priors keeps one per hypothesis for the next so_icp_register_batch call (batch.cpp).
#include <cmath>
#include <cstring>
#include <string>
#include <utility>

#include "ctx.h"
#include "pose_prior.h"

static_assert(sizeof(so_icp_pose_prior) == sizeof(PosePrior) && sizeof(so_icp_pose_prior) == kPosePriorWords * 8, "so_icp_pose_prior is pose_prior.h's PosePrior");
static_assert(offsetof(so_icp_pose_prior, sqrt_information) == kPriorU * 8 && offsetof(so_icp_pose_prior, count_floor) == kPriorFloor * 8 &&
              offsetof(so_icp_pose_prior, count_fraction) == kPriorFraction * 8, "so_icp_pose_prior's words are where pose_prior.h reads them");
static_assert(sizeof(so_icp_sums) == sizeof(LmSums), "so_icp_sums is LmSums");

extern "C" {

int so_icp_pose_prior_from_information(const double information[36], const double T_meas[7], so_icp_pose_prior* out) {
  if (!information || !T_meas || !out) return SO_ICP_E_INVALID;
  double U[36];
  if (!pose_prior_llt(information, U)) return SO_ICP_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  std::memcpy(out->T_meas, T_meas, sizeof(out->T_meas));
  std::memcpy(out->sqrt_information, U, sizeof(U));
  return SO_ICP_OK;
}

int so_icp_pose_prior_sums(const so_icp_pose_prior* prior, const double pose[7], so_icp_sums* inout) {
  if (!prior || !pose || !inout) return SO_ICP_E_INVALID;
  pose_prior_add(reinterpret_cast<const double*>(prior), pose, *reinterpret_cast<LmSums*>(inout));
  return SO_ICP_OK;
}

int so_icp_set_pose_prior(so_icp_ctx* c, const so_icp_pose_prior* prior) {
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (c->cfg.world_size > 1)
    return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_set_pose_prior: a sharded context (world_size > 1) sums every evaluation over the ranks; the prior belongs to one device");
  if (const int rc = refuse_pending_run_priors(c, "so_icp_set_pose_prior")) return rc;
  if (!prior) { c->prior_pending = false; return SO_ICP_OK; }
  const double* w = reinterpret_cast<const double*>(prior);
  for (int i = 0; i < kPosePriorWords; ++i)
    if (!std::isfinite(w[i])) return fail(c, SO_ICP_E_INVALID, "so_icp_set_pose_prior: a field of the prior is not finite");
  const double* q = prior->T_meas + 3;
  if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0)) return fail(c, SO_ICP_E_INVALID, "so_icp_set_pose_prior: T_meas holds a quaternion of zero norm");
  // host memory only: the prior is the last argument of the solve / evaluation launches of the registration that carries it
  std::memcpy(&c->prior, prior, sizeof(c->prior));
  c->prior_pending = true;
  return SO_ICP_OK;
}

}  // extern "C"

namespace {

// One prior and one mode per element (a frame of a run, a hypothesis of a batch), validated on the words its mode reads and copied
// into `next`; `entry`: the setter's name for the error text.  SO_ICP_OK, or SO_ICP_E_INVALID with c->err set and `next` to be dropped.
int copy_priors(so_icp_ctx* c, const std::string& entry, int count, const so_icp_pose_prior* priors, const uint8_t* modes, so_icp_ctx::RunPriors& next) {
  next.priors.resize((size_t)count);
  next.modes.assign((size_t)count, (uint8_t)SO_ICP_PRIOR_GIVEN);
  for (int k = 0; k < count; ++k) {
    const uint8_t mode = modes ? modes[k] : (uint8_t)SO_ICP_PRIOR_GIVEN;
    if (mode > SO_ICP_PRIOR_AT_GUESS) return fail(c, SO_ICP_E_INVALID, entry + ": modes[" + std::to_string(k) + "] is none of SO_ICP_PRIOR_*");
    next.modes[(size_t)k] = mode;
    PosePrior& P = next.priors[(size_t)k];
    if (mode == SO_ICP_PRIOR_NONE) { P = PosePrior{}; P.T_meas[6] = 1.0; continue; }  // (nothing of priors[k] is read)
    std::memcpy(&P, &priors[k], sizeof(P));
    if (mode == SO_ICP_PRIOR_AT_GUESS) { std::memset(P.T_meas, 0, sizeof(P.T_meas)); P.T_meas[6] = 1.0; }  // (not read: the element's guess takes its place)
    const double* w = reinterpret_cast<const double*>(&P);
    for (int i = 0; i < kPosePriorWords; ++i)
      if (!std::isfinite(w[i])) return fail(c, SO_ICP_E_INVALID, entry + ": a field of priors[" + std::to_string(k) + "] is not finite");
    const double* q = P.T_meas + 3;
    if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0))
      return fail(c, SO_ICP_E_INVALID, entry + ": priors[" + std::to_string(k) + "].T_meas holds a quaternion of zero norm");
  }
  next.pending = true;
  return SO_ICP_OK;
}

}  // namespace

extern "C" {

int so_icp_set_sequence_priors(so_icp_ctx* c, int count, const so_icp_pose_prior* priors, const uint8_t* modes) {
  if (!c || count < 0) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (c->cfg.world_size > 1)
    return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_set_sequence_priors: a sharded context (world_size > 1) sums every evaluation over the ranks; the prior belongs to one device");
  if (count == 0 || !priors) { c->run_priors = so_icp_ctx::RunPriors{}; return SO_ICP_OK; }
  if (const int rc = refuse_pending_prior(c, "so_icp_set_sequence_priors", true)) return rc;
  so_icp_ctx::RunPriors next;
  if (const int rc = copy_priors(c, "so_icp_set_sequence_priors", count, priors, modes, next)) return rc;
  c->run_priors = std::move(next);  // (a refused call leaves what was pending)
  return SO_ICP_OK;
}

int so_icp_set_batch_priors(so_icp_ctx* c, int n_hyp, const so_icp_pose_prior* priors, const uint8_t* modes) {
  if (!c || n_hyp < 0) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (c->cfg.world_size > 1)
    return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_set_batch_priors: so_icp_register_batch needs the whole map on one device (world_size == 1), and so do its priors");
  if (n_hyp == 0 || !priors) { c->batch_priors = so_icp_ctx::RunPriors{}; return SO_ICP_OK; }
  if (const int rc = refuse_pending_prior(c, "so_icp_set_batch_priors", false, true)) return rc;  // (a single prior, the priors of a run)
  so_icp_ctx::RunPriors next;
  if (const int rc = copy_priors(c, "so_icp_set_batch_priors", n_hyp, priors, modes, next)) return rc;
  c->batch_priors = std::move(next);  // (a refused call leaves what was pending)
  return SO_ICP_OK;
}

}  // extern "C"
