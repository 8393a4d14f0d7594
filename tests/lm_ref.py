"""A plain restatement of the trust-region Levenberg-Marquardt loop of ceres-solver 2.0.0 as the registration configures it
(TRUST_REGION / LEVENBERG_MARQUARDT, every other option default, jacobi_scaling on), driven by SCRIPTED evaluations: every
evaluation is an so_icp_sums record {cost, count, g = J^T r, H = J^T J, hist}, so no scene is needed and every branch can be
reached on purpose.  Written from the upstream semantics listed at the top of test_lm_branches.py, not from lm_solver.h:

  * it keeps the trust-region RADIUS and divides by it (lm_diagonal^2 = diagonal / radius);
  * the step quality is the cost change DIVIDED by the model cost change;
  * the damped, Jacobi-scaled 6x6 system (Hs + diag / radius) y = gs is solved by numpy in np.longdouble (64-bit mantissa:
    Gaussian elimination with partial pivoting, one step of refinement), not by a Cholesky factorisation.

Upstream, besides the lines cited in test_lm_branches.py:
  TrustRegionMinimizer::ComputeTrustRegionStep   model_cost_change = -(J s)^T (r + J s / 2); the step is valid iff that is > 0
  TrustRegionMinimizer::HandleInvalidStep        ++num_consecutive_invalid_steps; >= 5 -> FAILURE; else strategy->StepIsInvalid()
  LevenbergMarquardtStrategy::StepIsInvalid      (levenberg_marquardt_strategy.h) "Treat the current step as a rejected step with
                                                 no increase in solution quality": StepRejected(0.0) -- radius /= decrease_factor,
                                                 decrease_factor *= 2, the diagonal is reused
  LevenbergMarquardtStrategy::ComputeStep        diagonal = clamp(squared column norms of the SCALED Jacobian, 1e-6, 1e32) unless reused
  TrustRegionMinimizer::MinTrustRegionRadiusReached   radius <= 1e-32, tested before every iteration
DENSE_QR on the stacked [J; D] cannot fail on a true J^T J; for a scripted H that is not positive definite "the linear solver
failed" is restated as: the damped matrix is not positive definite, or the solution is not finite.

Scripted quantities are compared the way upstream compares them, in IEEE double (the function tolerance is one product and one
difference of two scripted costs: exact on every side); whatever depends on a solved step is formed in np.longdouble, and
every threshold comparison reports its MARGIN -- |quantity - threshold| / |threshold| -- so that a script can be required to
stay clear of every threshold that rounding could move."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

INITIAL_RADIUS, MAX_RADIUS, MIN_RADIUS = 1e4, 1e16, 1e-32
MIN_RELATIVE_DECREASE, MIN_LM_DIAGONAL, MAX_LM_DIAGONAL = 1e-3, 1e-6, 1e32
FUNCTION_TOLERANCE, GRADIENT_TOLERANCE, PARAMETER_TOLERANCE = 1e-6, 1e-10, 1e-8
MAX_CONSECUTIVE_INVALID_STEPS = 5


def full_H(JtJ21):
    H = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = JtJ21[k]; k += 1
    return H


def pose_plus(x, d, LD=LD):
    """PoseLocalParameterization::Plus: p += dp, q = normalize(q (x) [dtheta / 2, 1]); quaternion stored x y z w."""
    x = np.asarray(x, LD); d = np.asarray(d, LD)
    ax, ay, az, aw = x[3:7]
    dx, dy, dz = d[3:6] / LD(2)
    q = np.array([aw * dx + ax + ay * dz - az * dy,
                  aw * dy - ax * dz + ay + az * dx,
                  aw * dz + ax * dy - ay * dx + az,
                  aw - ax * dx - ay * dy - az * dz], LD)
    q = q / np.sqrt(np.sum(q * q))
    return np.concatenate([x[:3] + d[:3], q])


def relative_motion(a, b):
    """|(a^-1 b).t| and the rotation angle of a^-1 b (LidarSlam.cpp:246-249)."""
    a = np.asarray(a, LD); b = np.asarray(b, LD)
    tn = np.sqrt(np.sum((b[:3] - a[:3]) ** 2))   # a rotation does not change the length
    ax, ay, az, aw = -a[3], -a[4], -a[5], a[6]
    bx, by, bz, bw = b[3:7]
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                  aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], LD)
    return float(tn), float(2 * np.arctan2(np.sqrt(np.sum(q[:3] ** 2)), abs(q[3])))


def _margin(q, t):
    q = float(q); t = float(t)
    if not np.isfinite(q):
        return float("inf")
    return abs(q - t) / abs(t)


def _solve_ld(A, b):
    """x = A^-1 b in longdouble: LU with partial pivoting + one refinement step."""
    n = len(b)
    M = np.array(A, LD); perm = list(range(n)); L = np.eye(n, dtype=LD)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]; perm[k], perm[p] = perm[p], perm[k]
            L[[k, p], :k] = L[[p, k], :k]
        for i in range(k + 1, n):
            L[i, k] = M[i, k] / M[k, k]
            M[i, k:] = M[i, k:] - L[i, k] * M[k, k:]

    def lu_solve(r):
        y = np.zeros(n, LD); r = np.asarray(r, LD)[perm]
        for i in range(n):
            y[i] = r[i] - np.sum(L[i, :i] * y[:i])
        z = np.zeros(n, LD)
        for i in range(n - 1, -1, -1):
            z[i] = (y[i] - np.sum(M[i, i + 1:] * z[i + 1:])) / M[i, i]
        return z
    x = lu_solve(b)
    return x + lu_solve(np.asarray(b, LD) - np.asarray(A, LD) @ x)


class Solve:
    """One Minimize(): begin(x0, sums) then feed(sums) while `more`.  After every call `log` describes what was decided."""

    def __init__(self, max_iterations):
        self.max_iter = int(max_iterations)

    # ---- helpers
    def _gradient_max_norm(self, solved):
        # at the start x and g are both given: formed in double, as upstream forms it (a gradient below half an ulp of x does not move x)
        t = LD if solved else np.float64
        x = self.x.astype(t)
        return float(np.max(np.abs(x - pose_plus(x, -self.g.astype(t), t))))

    def _gradient_converged(self, solved):
        gmn = self._gradient_max_norm(solved)
        self.log["margins"].append(("gradient", _margin(gmn, GRADIENT_TOLERANCE), solved))
        self.log["gradient_max_norm"] = gmn
        return gmn <= GRADIENT_TOLERANCE

    def _finish(self, termination):
        self.termination = termination; self.done = True; self.log["termination"] = termination
        return self._out(0)

    def _out(self, more):
        self.log.update(more=more, iter=self.iter, num_successful=self.num_successful, invalid_steps=self.invalid_steps,
                        radius=self.radius, decrease_factor=self.decrease_factor, reuse_diagonal=self.reuse_diagonal,
                        x=self.x.copy(), cand=self.cand.copy(), x_cost=self.x_cost, diag=self.diag.copy(), scale=self.scale.copy(),
                        model_cost_change=self.model_cost_change, H=self.H.astype(np.float64), g=self.g.astype(np.float64))
        return more

    # ---- the loop
    def begin(self, x0, sums):
        self.log = {"decisions": [], "margins": [], "proposals": []}
        self.x = np.asarray(x0, LD).copy(); self.cand = self.x.copy()
        self.iter = 0; self.num_successful = 0; self.invalid_steps = 0; self.termination = 0; self.done = False
        self.radius = LD(INITIAL_RADIUS); self.decrease_factor = 2.0; self.reuse_diagonal = False
        self.model_cost_change = LD(0)
        self.count = float(sums["count"]); self.x_cost = float(sums["cost"]); self.initial_cost = self.x_cost
        self.H = np.asarray(sums["H"], LD); self.g = np.asarray(sums["g"], LD)
        self.scale = np.ones(6, LD); self.diag = np.zeros(6, LD)
        self.log["decisions"].append("begin")
        if not (self.count >= 1):   # a problem without residual blocks (LidarSlam.cpp:213-228): the count is a number of blocks
            self.log["decisions"].append("no_residuals")
            return self._finish(4)
        self.scale = LD(1) / (LD(1) + np.sqrt(np.diag(self.H)))   # jacobi_scaling, fixed at iteration 0
        self.x_norm = np.sqrt(np.sum(self.x * self.x))
        if self._gradient_converged(False):
            self.log["decisions"].append("gradient_converged")
            return self._finish(3)
        return self._propose()

    def feed(self, sums):
        self.log = {"decisions": [], "margins": [], "proposals": []}
        if self.done:
            return self._out(0)
        cand_cost = float(sums["cost"])
        step_norm = np.sqrt(np.sum((self.x - self.cand) ** 2))
        tol = LD(PARAMETER_TOLERANCE) * (self.x_norm + LD(PARAMETER_TOLERANCE))
        self.log["margins"].append(("parameter", _margin(step_norm, tol), True))
        if step_norm <= tol:
            self.log["decisions"].append("parameter_tolerance")
            return self._finish(2)
        # two scripted costs, compared in double as upstream does: one difference, one product
        cost_change = np.float64(self.x_cost) - np.float64(cand_cost)
        ftol = np.float64(FUNCTION_TOLERANCE) * np.float64(self.x_cost)
        self.log["margins"].append(("function", _margin(abs(cost_change), ftol) if ftol != 0 else float("inf"), False))
        self.log["cost_change"] = float(cost_change)
        if abs(cost_change) <= ftol:
            self.log["decisions"].append("function_tolerance")
            return self._finish(1)
        rel = LD(cost_change) / self.model_cost_change   # TrustRegionStepEvaluator::StepQuality (monotonic steps)
        self.log["relative_decrease"] = float(rel)
        self.log["margins"].append(("accept", _margin(rel, MIN_RELATIVE_DECREASE), True))
        if rel > MIN_RELATIVE_DECREASE:   # HandleSuccessfulStep + StepAccepted
            self.log["decisions"].append("accepted")
            self.x = self.cand.copy()
            self.x_norm = np.sqrt(np.sum(self.x * self.x)); self.x_cost = cand_cost
            self.H = np.asarray(sums["H"], LD); self.g = np.asarray(sums["g"], LD)
            self.num_successful += 1
            u = LD(2) * rel - LD(1)
            f = LD(1) - u * u * u
            self.log["margins"].append(("factor_third", _margin(f, 1.0 / 3.0), True))
            self.log["factor_clamped"] = bool(f < LD(1) / LD(3))
            self.log["factor_sensitivity"] = float(abs(6 * u * u * rel) / max(f, LD(1) / LD(3)))  # d ln(1/f) / d ln(rel)
            f = max(f, LD(1) / LD(3))
            self.radius = self.radius / f
            self.log["margins"].append(("max_radius", _margin(self.radius, MAX_RADIUS), True))
            self.log["radius_clamped"] = bool(self.radius > MAX_RADIUS)
            self.radius = min(LD(MAX_RADIUS), self.radius)
            self.decrease_factor = 2.0; self.reuse_diagonal = False
            if self.iter >= self.max_iter:   # MaxSolverIterationsReached is tested before GradientToleranceReached
                self.log["decisions"].append("max_iterations")
                return self._finish(0)
            if self._gradient_converged(True):
                self.log["decisions"].append("gradient_converged")
                return self._finish(3)
        else:   # StepRejected
            self.log["decisions"].append("rejected")
            self.radius = self.radius / LD(self.decrease_factor); self.decrease_factor *= 2.0; self.reuse_diagonal = True
        return self._propose()

    def _propose(self):
        while True:
            if self.iter >= self.max_iter:
                self.log["decisions"].append("max_iterations")
                return self._finish(0)
            self.log["margins"].append(("min_radius", _margin(self.radius, MIN_RADIUS), False))
            if self.radius <= MIN_RADIUS:
                self.log["decisions"].append("min_radius")
                return self._finish(5)
            self.iter += 1
            prop = {"radius": float(self.radius)}
            self.log["proposals"].append(prop)
            if not self.reuse_diagonal:
                raw = np.diag(self.H) * self.scale * self.scale   # squared column norms of the scaled Jacobian
                prop["diag_floor"] = [bool(v < MIN_LM_DIAGONAL) for v in raw]
                self.diag = np.minimum(np.maximum(raw, LD(MIN_LM_DIAGONAL)), LD(MAX_LM_DIAGONAL))
                for v in raw:
                    self.log["margins"].append(("min_diagonal", _margin(v, MIN_LM_DIAGONAL), False))
            self.reuse_diagonal = True
            Hs = self.H * np.outer(self.scale, self.scale)
            gs = self.g * self.scale
            A = Hs + np.diag(self.diag / self.radius)
            valid = bool(np.all(np.isfinite(A.astype(np.float64))) and np.all(np.isfinite(gs.astype(np.float64))))
            why = "not_finite"
            if valid:
                ev = np.linalg.eigvalsh(A.astype(np.float64))
                prop["kappa"] = float(np.linalg.cond(A.astype(np.float64)))
                self.log["margins"].append(("positive_definite", abs(ev[0]) / max(abs(ev[-1]), 1e-300), True))
                # the first pivot that is not positive: which column a Cholesky factorisation stops at
                prop["first_bad_pivot"] = next((k for k in range(6) if np.linalg.eigvalsh(A[:k + 1, :k + 1].astype(np.float64))[0] <= 0), None)
                valid = bool(ev[0] > 0); why = "not_positive_definite"
            if valid:
                y = _solve_ld(A, gs)
                valid = bool(np.all(np.isfinite(y.astype(np.float64)))); why = "not_finite"
            if valid:
                step = -y
                mcc = -(step @ gs) - LD(0.5) * (step @ (Hs @ step))
                prop["model_cost_change"] = float(mcc)
                valid = bool(mcc > 0); why = "model_cost_change"
            prop["valid"] = valid
            if not valid:   # HandleInvalidStep; LevenbergMarquardtStrategy::StepIsInvalid == StepRejected(0)
                prop["invalid_because"] = why
                self.log["decisions"].append("invalid_step")
                self.invalid_steps += 1
                if self.invalid_steps >= MAX_CONSECUTIVE_INVALID_STEPS:
                    self.log["decisions"].append("invalid_failure")
                    return self._finish(5)
                self.radius = self.radius / LD(self.decrease_factor); self.decrease_factor *= 2.0
                continue
            self.invalid_steps = 0
            self.model_cost_change = mcc
            delta = step * self.scale
            self.cand = pose_plus(self.x, delta)
            prop["delta_norm"] = float(np.sqrt(np.sum(delta * delta)))
            prop["cand_norm"] = float(np.sqrt(np.sum(self.cand * self.cand)))
            self.log["decisions"].append("propose")
            return self._out(1)


def run_script(script):
    """script: dict(x0, lm_max, max_outer, outer_iter, entries=[dict(cost, count, g, H, hist, new_solve)]).
    Returns (per-entry logs, final outer state) with the outer ICP bookkeeping of LidarSlam.cpp:119-148, 242-251."""
    T = np.asarray(script["x0"], LD).copy()
    outer = int(script["outer_iter"]); max_outer = int(script["max_outer"])
    out = {"iters": {}, "reg_done": 0, "done_count": 0, "T_final": None, "JtJ": np.zeros((6, 6)), "Jtr": np.zeros(6), "n_iterations": outer}
    logs = []; solve = None; running = False
    for e in script["entries"]:
        if out["reg_done"] or not (e["new_solve"] or running):
            logs.append({"skipped": True, "more": 0, "decisions": [], "margins": [], "proposals": []}); continue
        if e["new_solve"]:
            solve = Solve(script["lm_max"]); T_start = T.copy()
            more = solve.begin(T, e)
        else:
            more = solve.feed(e)
        log = solve.log; log["skipped"] = False; logs.append(log)
        running = bool(more)
        if not more:
            T = solve.x.copy()
            tn, rn = relative_motion(T_start, T)
            out["iters"][min(outer, 15)] = dict(translation_norm=tn, rotation_norm=rn, num_surf=int(solve.count) if np.isfinite(solve.count) else None,
                                                lm_iterations=solve.iter, num_successful=solve.num_successful, termination=solve.termination,
                                                initial_cost=solve.initial_cost, final_cost=solve.x_cost, hist=[int(h) for h in e["hist"]],
                                                pose_after=T.copy())
            outer += 1; out["n_iterations"] = outer
            log["solve_end"] = True
            if solve.num_successful == 1 or outer >= max_outer:   # LidarSlam.cpp:141
                out["reg_done"] = 1; out["done_count"] += 1; out["T_final"] = T.copy()
                if solve.count >= 1:
                    out["JtJ"] = solve.H.astype(np.float64); out["Jtr"] = solve.g.astype(np.float64)
    out["T"] = T; out["outer_iter"] = outer; out["solve"] = solve; out["lm_more"] = int(running)
    return logs, out


def pose_bound(C, kappa, delta_norm, x_norm):
    """|cand_double - cand_reference| per proposal: the solved step (conditioning x step length) + the rounding of the pose itself."""
    return C * EPS * kappa * delta_norm + 4 * EPS * x_norm
