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

}  // extern "C"

namespace {

// Every word of `P` is finite and its T_meas holds a quaternion: SO_ICP_OK, or SO_ICP_E_INVALID with its text, which names element k
// of a setter's list as priors[k] (k < 0: the one prior of so_icp_set_pose_prior)
int validate_prior(so_icp_ctx* c, const char* entry, const PosePrior& P, int k) {
  const double* w = reinterpret_cast<const double*>(&P);
  bool finite = true;
  for (int i = 0; i < kPosePriorWords; ++i) finite = finite && std::isfinite(w[i]);
  const double* q = P.T_meas + 3;
  if (finite && q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0) return SO_ICP_OK;
  const std::string element = k < 0 ? "" : "priors[" + std::to_string(k) + "]";
  return fail(c, SO_ICP_E_INVALID, std::string(entry) + (!finite ? ": a field of " + (k < 0 ? "the prior" : element) + " is not finite"
                                                                 : ": " + (k < 0 ? "T_meas" : element + ".T_meas") + " holds a quaternion of zero norm"));
}

// so_icp_set_sequence_priors, so_icp_set_batch_priors (`kind`, `entry`; `sharded_text`: what a context of world_size > 1 answers): one
// prior and one mode per element -- a frame of a run, a hypothesis of a batch --, validated on the words its mode reads
int set_priors(so_icp_ctx* c, PriorKind kind, const char* entry, const char* sharded_text, int count, const so_icp_pose_prior* priors,
               const uint8_t* modes) {
  if (!c || count < 0) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (c->cfg.world_size > 1) return fail(c, SO_ICP_E_UNSUPPORTED, std::string(entry) + sharded_text);
  if (count == 0 || !priors) { c->pending.withdraw(kind); return SO_ICP_OK; }  // (before the refusal: another kind stays, and the call is SO_ICP_OK)
  if (const int rc = refuse_pending(c, entry, kind)) return rc;
  PriorSet next;  // (built aside: a refused call leaves what was pending)
  next.kind = kind;
  next.priors.resize((size_t)count);
  next.modes.assign((size_t)count, (uint8_t)SO_ICP_PRIOR_GIVEN);
  for (int k = 0; k < count; ++k) {
    const uint8_t mode = modes ? modes[k] : (uint8_t)SO_ICP_PRIOR_GIVEN;
    if (mode > SO_ICP_PRIOR_AT_GUESS) return fail(c, SO_ICP_E_INVALID, std::string(entry) + ": modes[" + std::to_string(k) + "] is none of SO_ICP_PRIOR_*");
    next.modes[(size_t)k] = mode;
    PosePrior& P = next.priors[(size_t)k];
    if (mode == SO_ICP_PRIOR_NONE) { P = PosePrior{}; P.T_meas[6] = 1.0; continue; }  // (nothing of priors[k] is read)
    std::memcpy(&P, &priors[k], sizeof(P));
    if (mode == SO_ICP_PRIOR_AT_GUESS) { std::memset(P.T_meas, 0, sizeof(P.T_meas)); P.T_meas[6] = 1.0; }  // (not read: the element's guess takes its place)
    if (const int rc = validate_prior(c, entry, P, k)) return rc;
  }
  c->pending = std::move(next);
  return SO_ICP_OK;
}

}  // namespace

extern "C" {

int so_icp_set_pose_prior(so_icp_ctx* c, const so_icp_pose_prior* prior) {
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (c->cfg.world_size > 1)
    return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_set_pose_prior: a sharded context (world_size > 1) sums every evaluation over the ranks; the prior belongs to one device");
  if (const int rc = refuse_pending(c, "so_icp_set_pose_prior", kPriorSingle)) return rc;  // (in front of the withdrawal too)
  if (!prior) { c->pending.withdraw(kPriorSingle); return SO_ICP_OK; }
  PosePrior P;
  std::memcpy(&P, prior, sizeof(P));
  if (const int rc = validate_prior(c, "so_icp_set_pose_prior", P, -1)) return rc;
  // host memory only: the prior is the last argument of the solve / evaluation launches of the registration that carries it
  c->pending.single = P;
  c->pending.kind = kPriorSingle;
  return SO_ICP_OK;
}

int so_icp_set_sequence_priors(so_icp_ctx* c, int count, const so_icp_pose_prior* priors, const uint8_t* modes) {
  return set_priors(c, kPriorsRun, "so_icp_set_sequence_priors",
                    ": a sharded context (world_size > 1) sums every evaluation over the ranks; the prior belongs to one device", count, priors, modes);
}

int so_icp_set_batch_priors(so_icp_ctx* c, int n_hyp, const so_icp_pose_prior* priors, const uint8_t* modes) {
  return set_priors(c, kPriorsBatch, "so_icp_set_batch_priors",
                    ": so_icp_register_batch needs the whole map on one device (world_size == 1), and so do its priors", n_hyp, priors, modes);
}

}  // extern "C"
