"""The host LM controller (so_icp_lm_begin / _feed: lm_solver.h) on every script of lm_script_data.py against the longdouble
restatement of the Ceres 2.0.0 trust-region loop (lm_ref.py) -- and the conditions the scripts themselves must meet, enforced on
the reference alone: every declared branch is reached, every threshold comparison that depends on a solved step keeps a margin
>= 1e-4, kappa2 <= 1e8 wherever a pose is compared, every branch named in REQUIRED has a script.

The positive-definite test of the damped matrix is not a comparison of a solved step: a Cholesky pivot of a 6x6 matrix is formed
with an error below 10 eps |A| ~ 2e-15 |A|, so a smallest eigenvalue of 1e-6 |A| (required below) is nine orders clear of it.

Pose bound C eps kappa2 |delta| + 4 eps |x| per proposal (lm_script_run.py).  Measured here, host form against the reference,
over every proposal of every script whose step term is at least its rounding term: largest ratio 0.1034 (invalid_run_4, entry 0);
C_MEASURED = 0.104, C = 8 x 0.104 = 0.832.  (Where the rounding term is the larger one the ratio only measures the rounding of the
pose itself -- up to 1e10 at |x| = 2e5 with a step of 1e-5 -- which the second term covers.)

What the scripts found: an invalid step (failed factorisation or model cost change <= 0) halved the radius every time and left
decrease_factor alone; upstream's LevenbergMarquardtStrategy::StepIsInvalid is StepRejected(0): radius / 2, / 4, / 8 ... like a
rejected step.  invalid_run_2, _3, _4, invalid_counter_reset and invalid_runs_use_up_the_iterations fail on the old rule.  And a
count of 1e-300 did not give termination 4 (the test was count > 0; it is count >= 1 now: the count is a number of blocks)."""
import numpy as np
import pytest

import lm_script_data as D
import lm_script_run as R
from superodom_amd import synth

SCRIPTS = {s["name"]: s for s in D.scripts()}
# every branch the scripts are there for (lm_script_data.branches_reached)
REQUIRED = ["no_residuals", "begin_gradient_zero", "begin_gradient_full_converged", "begin_gradient_full_not_converged", "begin_large_x_blocks_fast_exit",
            "parameter_tolerance", "function_tolerance", "function_tolerance_equal", "function_tolerance_ulp_inside", "function_tolerance_ulp_outside",
            "accepted_unclamped", "radius_grows", "radius_shrinks", "accepted_clamped_third", "max_radius_clamp", "accepted_last_iteration_zero_gradient",
            "accepted_gradient_converged", "rejected", "rejected_x3", "rejected_then_accepted", "rejected_last_iteration", "max_iterations",
            "invalid_first_column", "invalid_last_pivot", "invalid_not_finite", "invalid_run_1", "invalid_run_2", "invalid_run_3", "invalid_run_4",
            "invalid_failure", "invalid_after_accept", "min_diagonal_zero", "min_diagonal_tiny", "min_radius",
            "two_solves", "reg_done_one_success", "reg_done_max_outer", "iters_15", "hist", "skipped_after_reg_done"]


def test_symbol_is_exported_and_the_abi_version_stays(soicp):
    L = soicp.load()
    assert hasattr(L, "so_icp_debug_lm_script") and "so_icp_debug_lm_script" in soicp.EXPORTED
    assert L.so_icp_abi_version() == 4
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    e = [(R.to_sums(soicp, SCRIPTS["function_tolerance"]["entries"][0]), True)]
    with pytest.raises(soicp.SoIcpError):   # no CPU fall-back: a host-only context has no device forms
        host.debug_lm_script(0, D.X0, e)
    with pytest.raises(soicp.SoIcpError):
        host.debug_lm_script(2, D.X0, e)
    with pytest.raises(soicp.SoIcpError):
        host.debug_lm_script(0, D.X0, e * 65)


def test_every_required_branch_has_a_script():
    declared = set(b for s in SCRIPTS.values() for b in s["branches"])
    assert set(REQUIRED) <= declared, sorted(set(REQUIRED) - declared)
    assert len(SCRIPTS) == len(D.scripts()), "script names are unique"


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_script_meets_its_conditions_on_the_reference(name):
    s = SCRIPTS[name]
    assert 1 <= len(s["entries"]) <= 64
    logs, out = R.run_ref(s)
    reached = D.branches_reached(s, logs, out)
    assert set(s["branches"]) <= reached, (name, sorted(set(s["branches"]) - reached), sorted(reached))
    for k, lg in enumerate(logs):
        for what, margin, solved in lg["margins"]:
            if what == "positive_definite":
                assert margin >= 1e-6, (name, k, what, margin)
            elif solved:
                assert margin >= 1e-4, (name, k, what, margin)
        if lg["more"]:
            assert [p for p in lg["proposals"] if p["valid"]][-1]["kappa"] <= 1e8, (name, k)


def test_exact_function_tolerance_edge_is_exact():
    x = np.float64(D.EXACT_COST); tol = np.float64(1e-6) * x
    assert tol == 2.0 ** -9 and x - (x - tol) == tol and (x - tol) + tol == x
    for nm, cmp in (("function_tolerance_equal", 0), ("function_tolerance_ulp_inside", -1), ("function_tolerance_ulp_outside", 1)):
        c = np.float64(SCRIPTS[nm]["entries"][1]["cost"])
        assert np.sign((x - c) - tol) == cmp


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_host_controller_follows_the_reference(soicp, name):
    s = SCRIPTS[name]
    rows, outer = R.run_host(soicp, s)
    logs, out = R.run_ref(s)
    R.check_against_ref(s, rows, logs)
    assert outer["outer_iter"] == out["outer_iter"] and outer["reg_done"] == out["reg_done"]
    if s["name"].startswith("no_residuals"):   # scale 1, diag 0, nothing adopted but the sums
        S = rows[0]["S"]
        assert np.all(S["scale"] == 1.0) and np.all(S["diag"] == 0.0) and np.array_equal(S["x"], s["x0"]) and S["lm_iterations"] == 0


def test_measured_constant_of_the_pose_bound(soicp):
    """The ratio C_MEASURED is the largest of (see the module docstring)."""
    worst = (0.0, None)
    for s in SCRIPTS.values():
        rows, _ = R.run_host(soicp, s); logs, _ = R.run_ref(s)
        for k, (row, lg) in enumerate(zip(rows, logs)):
            if row is None or not lg["more"]:
                continue
            p = [q for q in lg["proposals"] if q["valid"]][-1]
            step_part = R.EPS * p["kappa"] * p["delta_norm"]
            if step_part < 4 * R.EPS * p["cand_norm"]:
                continue
            S = row["S"]
            ec = float(np.linalg.norm(S["cand"].astype(np.longdouble) - lg["cand"])); ex = float(np.linalg.norm(S["x"].astype(np.longdouble) - lg["x"]))
            worst = max(worst, ((ec - ex) / step_part, f"{s['name']}[{k}]"))
    print("largest host / reference ratio of the step term:", worst)
    assert worst[1] is not None and worst[0] <= R.C_MEASURED, worst


def test_recorded_real_problems(soicp, oracle):
    """The four set-ups of test_lm_branches.py as scripts: the reference replays the recorded evaluations to the same decisions as the
    host controller that recorded them, and orc_lm_solve (QR on the stacked Jacobian) agrees on iterations, successes, termination."""
    seen = set()
    for s, (pose_o, st_o) in D.real_scripts(soicp, oracle):
        rows, _ = R.run_host(soicp, s)
        logs, out = R.run_ref(s)
        R.check_against_ref(s, rows, logs)
        S = rows[-1]["S"]
        assert (S["lm_iterations"], S["num_successful"], S["termination"]) == (st_o.lm_iterations, st_o.num_successful_steps, st_o.termination), s["name"]
        dt, dr = synth.pose_error(S["x"], pose_o)
        assert dt < 1e-9 and dr < 1e-9, (s["name"], dt, dr)
        assert len(s["entries"]) == 1 + st_o.lm_iterations
        seen |= D.branches_reached(s, logs, out)
    # (no rejected step among them: not one of the 40 starts of test_rejected_step_shrinks_the_radius_and_retries has one)
    assert {"max_iterations", "parameter_tolerance", "function_tolerance", "accepted_clamped_third"} <= seen, sorted(seen)
