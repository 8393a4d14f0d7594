// pose_prior.h -- the absolute pose prior of the reference's Ceres problem, as a contribution to the sums the LM controller reads.
//   SE3AbsolutatePoseFactor::Evaluate          src/LidarProcess/SE3AbsolutatePoseFactor.cpp:9-51
//   LidarSLAM::addAbsolutePoseConstraints      src/LidarProcess/LidarSlam.cpp:285-297 (the information matrix, scaled by the feature count)
//   PoseLocalParameterization::ComputeJacobian [I6; 0]: the local Jacobian is the first six columns of the 6x7 global one
// One 6-row residual block at a pose {t, q = x y z w}:
//   e[0..2] = t - t_m,  qe = conj(q_m) (x) q,  e[3..5] = 2 vec(qe)            (qe as it is)
//   B = blockdiag(I3, w' I3 + [v']x),  (v', w') = qe, negated when qe.w < 0      (Utility::Qleft's positify: in the Jacobian only)
//   d_k = sqrt(max(count_floor[k], trunc(count * count_fraction[k]))) where count_floor[k] > 0, else 1
//   r = D U e,  J = D (U B);   cost += r'r / 2,  Jtr += J'r,  JtJ += J'J (upper triangle, LmSums order); count and hist stay
// Every output word is ONE fixed left-to-right chain of the operations written here (SO_FMA where lm_solver.h uses it), formed
// without reference to any other word: the host adds the 28 words one after the other, the device one word per lane, and both
// give the same bits.  A word's work comes in two parts: what needs the pose alone (pose_prior_prepare: the rows of U e and the two
// columns of U B the word reads) and what needs the count as well (pose_prior_finish) -- on the device the first part runs in
// front of the wait for the pass's last record.
// The measurement T_meas may lie apart from the other 48 words (so_icp_set_sequence_priors, SO_ICP_PRIOR_AT_GUESS: the frame's guess,
// DevState::pose_in, with U / floor / fraction from the kernel's argument): the *_at forms take it as a pointer of its own, and the
// forms without it are those with Tm = P -- the same chains on the same operands.
#pragma once
#include "lm_solver.h"
#include "so_math.h"

#if defined(__HIP__)
#define SO_PRIOR_UNROLL _Pragma("unroll")
#else
#define SO_PRIOR_UNROLL
#endif

namespace soicp {

// == so_icp_pose_prior (include/so_icp.h), 55 doubles; the functions below read it through a pointer to its first word
struct PosePrior {
  double T_meas[7];
  double U[36];  // row-major, residual = U e
  double count_floor[6], count_fraction[6];
};
constexpr int kPosePriorWords = 55, kPriorU = 7, kPriorFloor = 43, kPriorFraction = 49;
static_assert(sizeof(PosePrior) == kPosePriorWords * 8, "PosePrior is 55 doubles");
constexpr int kPriorSumWords = 29;  // cost, count, Jtr[6], JtJ[21]: the words of LmSums in front of hist

// word of LmSums -> the columns (i, j) of J it reads: word 0 (cost) and 1 (count) none, 2 + i: Jtr[i], 8 + t: entry t of the upper triangle
SO_HD void pose_prior_columns(int word, int& i, int& j) {
  if (word < 8) { i = word >= 2 ? word - 2 : 0; j = i; return; }
  const int t = word - 8;
  i = (t >= 6) + (t >= 11) + (t >= 15) + (t >= 18) + (t >= 20);
  j = i + t - (6 * i - (i * (i - 1)) / 2);
}

// the residual e and the rotation block's quaternion (v', w') at `pose`; Tm: the measurement's seven words
SO_HD void pose_prior_error(const double* Tm, const double pose[7], double e[6], double m[4]) {
  e[0] = pose[0] - Tm[0]; e[1] = pose[1] - Tm[1]; e[2] = pose[2] - Tm[2];
  const double qc[4] = {-Tm[3], -Tm[4], -Tm[5], Tm[6]};
  double qe[4];
  quat_mul(qc, pose + 3, qe);
  e[3] = 2.0 * qe[0]; e[4] = 2.0 * qe[1]; e[5] = 2.0 * qe[2];
  const bool neg = qe[3] < 0.0;
  m[0] = neg ? -qe[0] : qe[0]; m[1] = neg ? -qe[1] : qe[1]; m[2] = neg ? -qe[2] : qe[2]; m[3] = neg ? -qe[3] : qe[3];
}

// column c of U B, row by row: U's own column for a translation column (B's is a unit vector), the chain over the rotation block
// w' I + [v']x = [w' -z' y'; z' w' -x'; -y' x' w'] for a rotation column
SO_HD void pose_prior_column(const double* P, const double m[4], int c, double col[6]) {
  const bool rot = c >= 3;
  const int cr = rot ? c - 3 : 0;
  const double m0 = cr == 0 ? m[3] : (cr == 1 ? -m[2] : m[1]);
  const double m1 = cr == 0 ? m[2] : (cr == 1 ? m[3] : -m[0]);
  const double m2 = cr == 0 ? -m[1] : (cr == 1 ? m[0] : m[3]);
  SO_PRIOR_UNROLL
  for (int k = 0; k < 6; ++k) {
    const double* u = P + kPriorU + 6 * k;
    const double chain = SO_FMA(u[5], m2, SO_FMA(u[4], m1, u[3] * m0));
    col[k] = rot ? chain : u[c];
  }
}

// what a word needs besides the count: the rows of U e, columns i and j of U B, and the rows' floor and fraction (fetched with the
// rest, so that nothing is read from memory once the count is known)
struct PosePriorPart { double ue[6], ci[6], cj[6], floor[6], fraction[6]; };

// (Tm: T_meas; P: the prior's 55 words, of which the first seven are not read)
SO_HD void pose_prior_prepare_at(const double* Tm, const double* P, const double pose[7], int word, PosePriorPart& part) {
  double e[6], m[4];
  pose_prior_error(Tm, pose, e, m);
  int i, j;
  pose_prior_columns(word, i, j);
  SO_PRIOR_UNROLL
  for (int k = 0; k < 6; ++k) {
    const double* u = P + kPriorU + 6 * k;
    double s = u[0] * e[0];
    SO_PRIOR_UNROLL
    for (int c = 1; c < 6; ++c) s = SO_FMA(u[c], e[c], s);
    part.ue[k] = s;
  }
  pose_prior_column(P, m, i, part.ci);
  pose_prior_column(P, m, j, part.cj);
  SO_PRIOR_UNROLL
  for (int k = 0; k < 6; ++k) { part.floor[k] = P[kPriorFloor + k]; part.fraction[k] = P[kPriorFraction + k]; }
}

SO_HD void pose_prior_prepare(const double* P, const double pose[7], int word, PosePriorPart& part) { pose_prior_prepare_at(P, P, pose, word, part); }

// LidarSlam.cpp:289-294: information(k, k) carries std::max(floor, int(good_feature_num * fraction)); its square root scales row k
SO_HD double pose_prior_row_scale(double floor, double fraction, double count) {
  const double scaled = trunc(count * fraction);
  return floor > 0.0 ? sqrt(scaled > floor ? scaled : floor) : 1.0;
}

// the prior's contribution to word `word` (not 1) of the sums whose count word is `count`
SO_HD double pose_prior_finish(const PosePriorPart& part, double count, int word) {
  const bool is_cost = word == 0, is_jtr = word < 8;
  double s = 0;
  SO_PRIOR_UNROLL
  for (int k = 0; k < 6; ++k) {
    const double d = pose_prior_row_scale(part.floor[k], part.fraction[k], count);
    const double r = d * part.ue[k], ji = d * part.ci[k], jj = d * part.cj[k];
    s = SO_FMA(is_cost ? r : ji, is_jtr ? r : jj, s);
  }
  return is_cost ? 0.5 * s : s;
}

// host form: the 28 words one after the other, plane sum on the left of every addition
SO_HD void pose_prior_add_at(const double* Tm, const double* P, const double pose[7], LmSums& sums) {
  double* o = reinterpret_cast<double*>(&sums);
  const double count = sums.count;
  for (int word = 0; word < kPriorSumWords; ++word) {
    if (word == 1) continue;
    PosePriorPart part;
    pose_prior_prepare_at(Tm, P, pose, word, part);
    o[word] = o[word] + pose_prior_finish(part, count, word);
  }
}
SO_HD void pose_prior_add(const double* P, const double pose[7], LmSums& sums) { pose_prior_add_at(P, P, pose, sums); }

// U = L^T of the LLT of a symmetric positive semi-definite matrix (its lower triangle is read).  A zero pivot with a zero column
// below it is allowed (the reference's information(5,5) is 0) and leaves a zero row in U.  false: not such a matrix.
inline bool pose_prior_llt(const double info[36], double U[36]) {
  double L[36];
  for (int i = 0; i < 36; ++i) { L[i] = 0; U[i] = 0; }
  for (int j = 0; j < 6; ++j) {
    if (!(info[7 * j] >= 0.0)) return false;
    double d = info[7 * j];
    for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k];
    if (!(d >= 0.0) || !isfinite(d)) return false;
    const double ljj = sqrt(d);
    L[7 * j] = ljj;
    for (int i = j + 1; i < 6; ++i) {
      double s = info[6 * i + j];
      for (int k = 0; k < j; ++k) s -= L[6 * i + k] * L[6 * j + k];
      if (!isfinite(s)) return false;
      if (d == 0.0) { if (s != 0.0) return false; L[6 * i + j] = 0; }
      else L[6 * i + j] = s / ljj;
    }
  }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) U[6 * j + i] = L[6 * i + j];
  return true;
}

}  // namespace soicp
