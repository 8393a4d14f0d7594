"""Named scripts for the LM controllers (so_icp_lm_begin / _feed on the host, so_icp_debug_lm_script on the device): sequences of
so_icp_sums records that drive the controller through a chosen branch, with no scene.  A script is
    dict(name, branches, x0, lm_max, max_outer, outer_iter, entries=[dict(cost, count, g, H, hist, new_solve)])
`branches` are the branch tags (see branches_reached) the script is there for; tests/test_lm_scripts_host.py requires the
reference (tests/lm_ref.py) to reach every one of them, with margins.  Where a script needs a step of a given quality
rho = cost change / model cost change, the candidate's cost is formed from the REFERENCE's model cost change while the
script is built (a controller under test never contributes to a script).

Branch left without a script, and why: an invalid step by `model cost change <= 0` ALONE.  With y = A^-1 gs and
A = Hs + D (D = diag / radius > 0) the model cost change is y^T (Hs / 2 + D) y; if that is <= 0 for y != 0 then
y^T Hs y < -2 y^T D y, so y^T A y < 0 and A is not positive definite: the factorisation has failed already.  y = 0 needs
gs = 0, which ends the solve on the gradient tolerance before any step is proposed.  What is left is overflow of finite
inputs, which a longdouble reference does not reproduce.  The branch runs together with a failed factorisation in every
invalid_* script."""
import numpy as np

import lm_ref

X0 = np.r_[1.0, -2.0, 0.5, 0.0, 0.0, np.sin(0.2), np.cos(0.2)]
HIST_A = [3, 0, 1, 7, 0, 2, 5, 11, 13, 17, 19, 23, 29, 31, 37, 41]
HIST_B = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
EXACT_COST = 1953.125   # 1e-6 (as a double) x 1953.125 == 2^-9 exactly, and 1953.125 - 2^-9 is a double


def problem(seed, rows=40, residual=0.05):
    """H = J^T J, g = J^T r of a random, well-conditioned 6-parameter problem (translations and rotations of different weight)."""
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(rows, 6)) * np.r_[1.0, 1.0, 1.0, 6.0, 6.0, 6.0]
    r = rng.normal(size=rows) * residual
    return J.T @ J, J.T @ r


def E(cost, g, H, count=100.0, hist=None, new=False):
    return dict(cost=float(cost), count=count, g=np.array(g, np.float64), H=np.array(H, np.float64), hist=list(hist or [0] * 16), new_solve=bool(new))


class Builder:
    """Builds a script entry by entry beside the reference, so that `quality` can ask for a step of a given rho."""

    def __init__(self, name, branches, x0=X0, lm_max=12, max_outer=5, outer_iter=0):
        self.s = dict(name=name, branches=list(branches), x0=np.array(x0, np.float64), lm_max=lm_max, max_outer=max_outer, outer_iter=outer_iter, entries=[])

    def _ref(self):
        with np.errstate(all="ignore"):
            logs, out = lm_ref.run_script(self.s)
        return logs, out

    def add(self, *a, **k):
        self.s["entries"].append(E(*a, **k)); return self

    def quality(self, rho, g, H, **k):
        """The candidate's evaluation: its cost gives the step the quality rho (H, g are what the candidate's evaluation returns)."""
        _, out = self._ref()
        sv = out["solve"]
        return self.add(sv.x_cost - rho * float(sv.model_cost_change), g, H, **k)

    def same_cost(self, g, H, scale=1.0, **k):
        _, out = self._ref()
        return self.add(out["solve"].x_cost * scale, g, H, **k)

    def done(self):
        return self.s


def _pair_block(b, col=4, weight=4.0):
    """diag(weight) with one off-diagonal pair (col, col+1) = weight (1 + b): after Jacobi scaling the damped matrix is positive definite
    iff b < 1 / radius, and the pivot that fails is the one of column col + 1."""
    H = np.eye(6) * weight
    H[col, col + 1] = H[col + 1, col] = weight * (1.0 + b)
    return H


def build_scripts():
    S = []
    H1, g1 = problem(1); H2, g2 = problem(2); H3, g3 = problem(3)
    g_big = np.r_[0.3, -0.2, 0.25, 0.4, -0.5, 0.3]

    # ---------------- start of a solve
    for tag, cnt in (("zero", 0.0), ("tiny", 1e-300), ("negative", -3.0), ("nan", float("nan"))):
        S.append(Builder("no_residuals_" + tag, ["no_residuals", "reg_done_max_outer"], max_outer=1).add(7.5, g1, H1, count=cnt, hist=HIST_A, new=True).done())
    S.append(Builder("begin_gradient_zero", ["begin_gradient_zero"]).add(3.0, np.zeros(6), H1, new=True).done())
    S.append(Builder("begin_gradient_full_converged", ["begin_gradient_full_converged"])
             .add(3.0, [5e-11, -3e-11, 2e-11, 4e-11, -6e-11, 1e-11], H1, new=True).done())
    b = Builder("begin_gradient_rotation_keeps_going", ["begin_gradient_full_not_converged", "function_tolerance"])
    b.add(3.0, [5e-11, -3e-11, 2e-11, 1e-3, -2e-3, 5e-4], H1, new=True).same_cost(g2, H2)
    S.append(b.done())
    # |x[0]| >= 1e5: the fast exit must not fire although |g[0]| > 1e-6 -- x[0] - g[0] rounds back to x[0]: converged
    S.append(Builder("begin_large_x_full_test_converges", ["begin_large_x_blocks_fast_exit", "begin_gradient_full_converged"], x0=np.r_[1e11, X0[1:]])
             .add(3.0, [2e-6, 0, 0, 0, 0, 0], H1, new=True).done())
    b = Builder("begin_large_x_full_test_goes_on", ["begin_large_x_blocks_fast_exit", "begin_gradient_full_not_converged"], x0=np.r_[2e5, X0[1:]])
    b.add(3.0, [1e-5, 0, 0, 0, 0, 0], H1, new=True).same_cost(g2, H2)
    S.append(b.done())

    # ---------------- a candidate arrives
    d = np.full(6, 1e-9)
    b = Builder("parameter_before_function", ["parameter_tolerance"]).add(3.0, H1 @ d, H1, new=True).same_cost(g2, H2)
    S.append(b.done())
    b = Builder("function_tolerance", ["function_tolerance"]).add(3.0, g1, H1, new=True).same_cost(g2, H2, scale=1 - 5e-7)
    S.append(b.done())
    edge = EXACT_COST - 2.0 ** -9
    S.append(Builder("function_tolerance_equal", ["function_tolerance", "function_tolerance_equal"]).add(EXACT_COST, g1, H1, new=True).add(edge, g2, H2).done())
    S.append(Builder("function_tolerance_ulp_inside", ["function_tolerance", "function_tolerance_ulp_inside"])
             .add(EXACT_COST, g1, H1, new=True).add(np.nextafter(edge, np.inf), g2, H2).done())
    b = Builder("function_tolerance_ulp_outside", ["function_tolerance_ulp_outside", "max_iterations"], lm_max=1)
    b.add(EXACT_COST, g1, H1, new=True).add(np.nextafter(edge, -np.inf), g2, H2)   # the step is judged (and accepted), not stopped
    S.append(b.done())
    b = Builder("accepted_unclamped", ["accepted_unclamped", "radius_grows", "radius_shrinks", "function_tolerance"], lm_max=12)
    b.add(50.0, g1, H1, new=True).quality(0.5, g2, H2).quality(0.25, g3, H3).quality(0.8, g1, H1).same_cost(g2, H2)
    S.append(b.done())
    b = Builder("accepted_clamped_third", ["accepted_clamped_third", "function_tolerance"])
    b.add(50.0, g1, H1, new=True).quality(1.0, g2, H2).quality(0.97, g3, H3).same_cost(g1, H1)
    S.append(b.done())
    b = Builder("max_radius_clamp", ["max_radius_clamp", "accepted_clamped_third", "max_iterations"], lm_max=30)
    b.add(5000.0, g1, H1, new=True)
    for k in range(30):
        b.quality(1.0, *((g2, H2) if k % 2 == 0 else (g1, H1)))
    S.append(b.done())
    b = Builder("accepted_last_iteration_zero_gradient", ["accepted_last_iteration_zero_gradient", "max_iterations"], lm_max=1)
    b.add(50.0, g1, H1, new=True).quality(0.5, np.zeros(6), H2)
    S.append(b.done())
    b = Builder("accepted_then_gradient_converged", ["accepted_gradient_converged"], lm_max=4)
    b.add(50.0, g1, H1, new=True).quality(0.5, np.zeros(6), H2)
    S.append(b.done())
    # rejected candidates carry H2 / g3: a controller that adopts them, or recomputes the diagonal, hands on another pose
    b = Builder("rejected_once_then_accepted", ["rejected", "rejected_then_accepted", "function_tolerance"])
    b.add(50.0, g1, H1, new=True).quality(-0.5, g3, H2).quality(0.5, g2, H3).same_cost(g1, H1)
    S.append(b.done())
    b = Builder("rejected_three_then_accepted", ["rejected", "rejected_x3", "rejected_then_accepted", "function_tolerance"])
    b.add(0.5, g1, H1, new=True).quality(-0.5, g3, H2).quality(5e-4, g2, H3).quality(-3.0, g3, H2).quality(0.6, g2, H3).same_cost(g1, H1)
    S.append(b.done())
    b = Builder("rejected_on_last_iteration", ["rejected", "rejected_last_iteration", "max_iterations"], lm_max=2)
    b.add(50.0, g1, H1, new=True).quality(-0.5, g3, H2).quality(-0.5, g3, H2)
    S.append(b.done())

    # ---------------- the proposal loop
    Hneg = H1.copy(); Hneg[0, 0] = -4.0   # sqrt(H00) is NaN: scale, diagonal and the FIRST pivot are NaN, never > 0
    S.append(Builder("invalid_first_pivot", ["invalid_first_column", "invalid_failure"]).add(50.0, g_big, Hneg, new=True).done())
    S.append(Builder("invalid_last_pivot", ["invalid_last_pivot", "invalid_failure"]).add(50.0, g_big, _pair_block(1.0), new=True).done())
    Hinf = H1.copy(); Hinf[0, 1] = Hinf[1, 0] = np.inf
    S.append(Builder("invalid_not_finite", ["invalid_not_finite", "invalid_failure"]).add(50.0, g_big, Hinf, new=True).done())
    # n invalid steps, then a valid one: the radius goes 1e4, /2, /4, /8, /16 -> 1/radius = 1e-4, 2e-4, 8e-4, 6.4e-3, 0.1024
    for n, bb in ((1, 1.5e-4), (2, 5.5e-4), (3, 2.5e-3), (4, 3e-2)):
        b = Builder(f"invalid_run_{n}", [f"invalid_run_{n}", "invalid_last_pivot", "function_tolerance"], lm_max=12)
        b.add(50.0, g_big, _pair_block(bb), new=True).same_cost(g2, H2)
        S.append(b.done())
    # the counter of CONSECUTIVE invalid steps starts again after a valid step: 3 + 3 invalid steps do not add up to 5
    b = Builder("invalid_counter_reset", ["invalid_run_3", "invalid_after_accept", "function_tolerance"], lm_max=12)
    b.add(50.0, g_big, _pair_block(2.5e-3), new=True).quality(0.5, g_big, _pair_block(0.2, col=1)).same_cost(g2, H2)
    S.append(b.done())
    b = Builder("invalid_runs_use_up_the_iterations", ["invalid_run_3", "max_iterations"], lm_max=3)   # every round counts as an iteration
    b.add(50.0, g_big, _pair_block(3e-2), new=True)
    S.append(b.done())
    for tag, hjj in (("zero", 0.0), ("tiny", 1e-30)):
        Hs_ = H1 * 1e-8; Hs_[3, :] = 0; Hs_[:, 3] = 0; Hs_[3, 3] = hjj
        gs_ = g1 * 1e-8; gs_[3] = 2e-12
        b = Builder("min_diagonal_" + tag, ["min_diagonal_" + tag, "rejected", "function_tolerance"])
        b.add(1e-6, gs_, Hs_, new=True).quality(-0.5, g2, H2).quality(0.5, gs_, Hs_).same_cost(gs_, Hs_)
        S.append(b.done())
    # MinTrustRegionRadiusReached: 15 rejections (radius 1e4 / 2^120 < 1e-32); a gradient of 1e24 keeps every step above the
    # parameter tolerance although the damping grows to 1e27
    b = Builder("min_radius", ["min_radius", "rejected"], lm_max=20)
    b.add(50.0, [1e24, 0, 0, 0, 0, 0], np.eye(6), new=True)
    for k in range(15):
        b.quality(-0.5, g3, H2)
    S.append(b.done())

    # ---------------- outer bookkeeping
    b = Builder("two_solves_then_one_success", ["two_solves", "reg_done_one_success", "hist", "skipped_after_reg_done"], max_outer=5)
    b.add(50.0, g1, H1, new=True).quality(0.5, g2, H2).quality(0.5, g3, H3).same_cost(g1, H1, hist=HIST_A)
    b.add(40.0, g2, H2, new=True).quality(0.5, g3, H3).same_cost(g1, H1, hist=HIST_B)
    b.add(30.0, g1, H1, new=True).add(30.0, g1, H1)   # the registration is over: both are skipped
    S.append(b.done())
    b = Builder("reg_done_by_max_outer", ["two_solves", "reg_done_max_outer", "hist"], max_outer=2)
    b.add(50.0, g1, H1, new=True).quality(0.5, g2, H2).quality(0.5, g3, H3).same_cost(g1, H1, hist=HIST_A)
    b.add(40.0, g2, H2, new=True).quality(0.5, g3, H3).quality(0.5, g1, H1).same_cost(g1, H1, hist=HIST_B)
    S.append(b.done())
    b = Builder("outer_iter_17_writes_record_15", ["iters_15", "hist"], max_outer=30, outer_iter=17)
    b.add(50.0, g1, H1, new=True).quality(0.5, g2, H2).quality(0.5, g3, H3).same_cost(g1, H1, hist=HIST_B)
    S.append(b.done())
    return S


_CACHE = {}


def scripts():
    if "s" not in _CACHE:
        _CACHE["s"] = build_scripts()
    return _CACHE["s"]


REAL_SETUPS = (("real_max_iterations", 11, 0.01, (1, 0.3, 3.0), 2), ("real_gradient_parameter", 12, 0.0, (2, 0.05, 0.5), 12),
               ("real_function_tolerance", 13, 0.01, (3, 0.1, 1.0), 30), ("real_rejected_step", 14, 0.01, (100, 0.6, 25.0), 12))


def real_scripts(soicp, oracle):
    """The four problem set-ups of test_lm_branches.py, recorded by driving the HOST controller with oracle.evaluate.
    Returns [(script, (oracle pose, oracle stats))]."""
    if "real" in _CACHE:
        return _CACHE["real"]
    from superodom_amd import synth
    from test_oracle_numerics import _synthetic_corrs
    out = []
    for name, seed, noise, (pseed, dt, dr), lm_max in REAL_SETUPS:
        gt, corrs = _synthetic_corrs(oracle, np.random.default_rng(seed), noise=noise)
        x0 = None
        if name == "real_rejected_step":   # the start test_rejected_step_shrinks_the_radius_and_retries settles on (its condition, successes <
            # iterations, is met by the unapplied last step of a tolerance stop: none of its 40 starts has a rejected step)
            for k in range(40):
                x0 = synth.perturb_pose(gt, 100 + k, dt, dr)
                _, st = oracle.lm_solve(corrs, x0, 0.2, oracle.default_config(lm_max_iterations=lm_max))
                if 1 <= st.num_successful_steps < st.lm_iterations:
                    break
        else:
            x0 = synth.perturb_pose(gt, pseed, dt, dr)
        x0 = np.ascontiguousarray(x0, np.float64)
        entries = []
        drv = soicp.LmDriver()
        cost, JtJ, Jtr, cnt = oracle.evaluate(corrs, x0, 0.2)
        entries.append(E(cost, Jtr, JtJ, count=float(cnt), new=True))
        more, nxt = drv.begin(x0, soicp.LmDriver.sums(cost, cnt, Jtr, JtJ), lm_max)
        while more:
            cost, JtJ, Jtr, cnt = oracle.evaluate(corrs, nxt, 0.2)
            entries.append(E(cost, Jtr, JtJ, count=float(cnt)))
            more, nxt = drv.feed(soicp.LmDriver.sums(cost, cnt, Jtr, JtJ))
        script = dict(name=name, branches=[], x0=x0, lm_max=lm_max, max_outer=5, outer_iter=0, entries=entries)
        out.append((script, oracle.lm_solve(corrs, x0, 0.2, oracle.default_config(lm_max_iterations=lm_max))))
    _CACHE["real"] = out
    return out


def branches_reached(script, logs, out):
    """The branch tags the reference's run of `script` went through."""
    tags = set()
    solves = 0; run_rejected = 0; prev = None
    for e, lg in zip(script["entries"], logs):
        if lg.get("skipped"):
            if out["reg_done"]:
                tags.add("skipped_after_reg_done")
            continue
        dec = lg["decisions"]
        x = lg["x"].astype(np.float64)
        if dec[0] == "begin":
            solves += 1; run_rejected = 0
            g = e["g"]
            fast = any(abs(g[i]) > 1e-6 and abs(x[i]) < 1e5 for i in range(3))
            if "no_residuals" in dec:
                tags.add("no_residuals")
            elif not fast:
                if any(abs(g[i]) > 1e-6 and abs(x[i]) >= 1e5 for i in range(3)):
                    tags.add("begin_large_x_blocks_fast_exit")
                conv = "gradient_converged" in dec
                tags.add("begin_gradient_zero" if conv and not np.any(g) else ("begin_gradient_full_converged" if conv else "begin_gradient_full_not_converged"))
        for t in ("parameter_tolerance", "function_tolerance", "rejected", "max_iterations", "min_radius", "invalid_failure"):
            if t in dec:
                tags.add(t)
        if "function" in [m[0] for m in lg["margins"]] and "cost_change" in lg:
            cc = abs(lg["cost_change"]); ftol = np.float64(1e-6) * np.float64(prev["x_cost"] if prev else 0)
            if cc == ftol:
                tags.add("function_tolerance_equal")
            cand_ulp = np.spacing(np.float64(e["cost"]))
            if cc < ftol and cc + cand_ulp >= ftol and cc != ftol:
                tags.add("function_tolerance_ulp_inside")
            if cc > ftol and cc - cand_ulp <= ftol:
                tags.add("function_tolerance_ulp_outside")
        if "accepted" in dec:
            tags.add("accepted_clamped_third" if lg["factor_clamped"] else "accepted_unclamped")
            if not lg["factor_clamped"]:
                tags.add("radius_grows" if lg["radius"] > prev["radius"] else "radius_shrinks")
            if lg["radius_clamped"]:
                tags.add("max_radius_clamp")
            if run_rejected:
                tags.add("rejected_then_accepted")
            if not np.any(e["g"]):
                tags.add("accepted_last_iteration_zero_gradient" if "max_iterations" in dec else
                         ("accepted_gradient_converged" if "gradient_converged" in dec else "zero_gradient_not_converged"))
            run_rejected = 0
        if "rejected" in dec:
            run_rejected += 1
            if run_rejected >= 3:
                tags.add("rejected_x3")
            if "max_iterations" in dec:
                tags.add("rejected_last_iteration")
        n_inv = dec.count("invalid_step")
        if n_inv:
            if "propose" in dec or "max_iterations" in dec:
                tags.add(f"invalid_run_{n_inv}")
            if "accepted" in dec:
                tags.add("invalid_after_accept")
            for p in lg["proposals"]:
                if not p["valid"]:
                    if p["invalid_because"] == "not_finite":
                        tags.add("invalid_first_column" if not np.all(np.isfinite(np.sqrt(np.abs(np.diag(e["H"])))) & (np.diag(e["H"]) >= 0)) else "invalid_not_finite")
                    elif p.get("first_bad_pivot") == 5:
                        tags.add("invalid_last_pivot")
        for p in lg["proposals"]:
            for j, fl in enumerate(p.get("diag_floor", [])):
                if fl and lg["H"][j, j] == 0:
                    tags.add("min_diagonal_zero")
                if fl and lg["H"][j, j] == 1e-30:
                    tags.add("min_diagonal_tiny")
        if lg.get("solve_end"):
            if solves >= 2:
                tags.add("two_solves")
            if any(e["hist"]):
                tags.add("hist")
        prev = lg
    if out["reg_done"]:
        last = out["iters"][max(out["iters"])]
        tags.add("reg_done_one_success" if last["num_successful"] == 1 else "reg_done_max_outer")
    if script["outer_iter"] >= 16 and 15 in out["iters"]:
        tags.add("iters_15")
    return tags
