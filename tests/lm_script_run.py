"""Running the scripts of lm_script_data.py through the host controller (so_icp_lm_begin / _feed) and judging any double-precision
form of the controller -- host or device -- against the longdouble reference (lm_ref.py).  Shared by test_lm_scripts_host.py and
test_gpu_lm_scripts.py."""
import numpy as np

import lm_ref

EPS = lm_ref.EPS
# LmState (superodom_amd/csrc/lm_solver.h) as the first 656 bytes of so_icp_lm_state
LMSTATE = np.dtype([("x", "f8", 7), ("cand", "f8", 7), ("H", "f8", (6, 6)), ("g", "f8", 6), ("scale", "f8", 6), ("diag", "f8", 6),
                    ("x_cost", "f8"), ("x_norm", "f8"), ("inv_radius", "f8"), ("decrease_factor", "f8"), ("model_cost_change", "f8"),
                    ("initial_cost", "f8"), ("count", "f8"), ("inv_model_cost_change", "f8"), ("step_norm", "f8"), ("cand_norm", "f8"),
                    ("iter", "i4"), ("max_iter", "i4"), ("reuse_diagonal", "i4"), ("invalid_steps", "i4"), ("num_successful", "i4"),
                    ("termination", "i4"), ("done", "i4"), ("lm_iterations", "i4")])
assert LMSTATE.itemsize == 656
INT_FIELDS = ("iter", "max_iter", "reuse_diagonal", "invalid_steps", "num_successful", "termination", "done", "lm_iterations")
# never touched by a solved step: the same bits in every double-precision form
EXACT_FIELDS = ("x_cost", "initial_cost", "count", "decrease_factor", "H", "g", "scale", "diag")

# Pose bound, per proposal: C eps kappa2(A) |delta| + 4 eps |cand| (+ what the pose the step started from carries).
# C_MEASURED: the largest (|cand_host - cand_ref| - |x_host - x_ref| - 4 eps |cand|) / (eps kappa2 |delta|) over every proposal of every
# script, host form (Cholesky with 1 / sqrt) against the longdouble reference, measured on the CPU (test_lm_scripts_host.py prints
# and asserts it).  C = 8 x that, for the device's rsqrt and re-association; never read off the device output.
C_MEASURED = 0.104
C_BOUND = 8.0 * C_MEASURED


def decode_state(raw):
    return np.frombuffer(bytes(raw), dtype=LMSTATE, count=1)[0].copy()


def to_sums(soicp, e):
    return soicp.LmDriver.sums(e["cost"], e["count"], e["g"], e["H"], e["hist"])


def run_host(soicp, script):
    """Per entry: None (skipped) or dict(more, pose, S); plus the outer state the host emulation ends with."""
    T = np.array(script["x0"], np.float64); outer = script["outer_iter"]; reg_done = False; running = False; drv = None
    rows = []
    for e in script["entries"]:
        if reg_done or not (e["new_solve"] or running):
            rows.append(None); continue
        if e["new_solve"]:
            drv = soicp.LmDriver()
            more, nxt = drv.begin(T, to_sums(soicp, e), script["lm_max"])
        else:
            more, nxt = drv.feed(to_sums(soicp, e))
        S = decode_state(drv.s)
        rows.append(dict(more=more, pose=nxt, S=S))
        running = bool(more)
        if not more:
            T = S["x"].copy(); outer += 1
            reg_done = bool(S["num_successful"] == 1 or outer >= script["max_outer"])
    return rows, dict(T=T, outer_iter=outer, reg_done=int(reg_done))


def run_ref(script):
    with np.errstate(all="ignore"):
        return lm_ref.run_script(script)


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_bits_or_nan(a, b):
    """same_bits, except that a NaN may carry any payload and sign (x86 and gfx950 produce different default NaNs)."""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return same_bits(a, b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and same_bits(np.where(nan, 0.0, a), np.where(nan, 0.0, b))


def check_against_ref(script, rows, logs, C=C_BOUND, measure=None):
    """rows: per entry None or dict(more, S[, pose]) of a double-precision controller.  Every discrete field equals the reference's;
    poses and continuous state stay inside the bound.  measure: a list that receives the ratio described at C_MEASURED."""
    name = script["name"]
    x_bound = cand_bound = carry = radius_tol = 0.0; accepted_in_solve = 0
    for k, (row, lg) in enumerate(zip(rows, logs)):
        at = f"{name}[{k}]"
        assert (row is None) == bool(lg.get("skipped")), at
        if row is None:
            continue
        S = row["S"]
        if lg["decisions"][0] == "begin":   # a later solve starts from the pose the solve before ended with, and inherits its bound
            x_bound = cand_bound = carry; radius_tol = 0.0; accepted_in_solve = 0
        # ---- discrete
        assert row["more"] == lg["more"], (at, row["more"], lg["more"], lg["decisions"])
        assert S["iter"] == lg["iter"] == S["lm_iterations"], (at, S["iter"], lg["iter"])
        assert S["num_successful"] == lg["num_successful"], at
        assert S["invalid_steps"] == lg["invalid_steps"], (at, S["invalid_steps"], lg["invalid_steps"])
        assert S["done"] == (0 if lg["more"] else 1), at
        if not lg["more"]:
            assert S["termination"] == lg["termination"], (at, S["termination"], lg["termination"], lg["decisions"])
        assert S["decrease_factor"] == lg["decrease_factor"], (at, S["decrease_factor"], lg["decrease_factor"])
        if lg["proposals"]:
            assert S["reuse_diagonal"] == 1, at
        # ---- scripted quantities: exact
        assert S["x_cost"] == lg["x_cost"], at
        assert same_bits(S["H"], lg["H"]) and same_bits(S["g"], lg["g"]), (at, "held normal equations")
        np.testing.assert_allclose(S["scale"], lg["scale"].astype(np.float64), rtol=8 * EPS, atol=0, err_msg=at)
        np.testing.assert_allclose(S["diag"], lg["diag"].astype(np.float64), rtol=8 * EPS, atol=0, err_msg=at)
        # ---- radius
        if "accepted" in lg["decisions"]:
            accepted_in_solve += 1
            kap = max([p.get("kappa", 1.0) for p in logs[k - 1]["proposals"] if p.get("valid")] or [1.0])
            radius_tol += (lg["factor_sensitivity"] * 2 * C * kappa_eps(kap) + 8 * EPS) if not lg["radius_clamped"] else 0.0
            if lg["radius_clamped"]:
                radius_tol = 0.0   # clamped to the constant
            x_bound = cand_bound
        inv_ref = np.longdouble(1) / lg["radius"]
        if accepted_in_solve == 0:
            assert S["inv_radius"] == np.float64(inv_ref), (at, "1 / radius after rejections only: 1e-4 x a power of two, exact", S["inv_radius"], float(inv_ref))
        else:
            assert abs(S["inv_radius"] - inv_ref) <= (radius_tol + 2 * EPS) * inv_ref, (at, S["inv_radius"], float(inv_ref), radius_tol)
        # ---- poses
        ex = float(np.linalg.norm(S["x"].astype(np.longdouble) - lg["x"]))
        assert ex <= x_bound, (at, "x", ex, x_bound)
        if lg["more"]:
            p = [q for q in lg["proposals"] if q["valid"]][-1]
            assert p["kappa"] <= 1e8, (at, "a pose is compared at kappa", p["kappa"])
            step_part = EPS * p["kappa"] * p["delta_norm"]
            cand_bound = x_bound + C * step_part + 4 * EPS * p["cand_norm"]
            ec = float(np.linalg.norm(S["cand"].astype(np.longdouble) - lg["cand"]))
            if measure is not None and step_part > 0:
                measure.append((max(0.0, ec - ex - 4 * EPS * p["cand_norm"]) / step_part, at))
            assert ec <= cand_bound, (at, "candidate", ec, cand_bound)
            if "pose" in row:
                assert same_bits(np.asarray(row["pose"], np.float64), S["cand"]), (at, "the pose handed on is the candidate")
            mref = float(lg["model_cost_change"])
            assert abs(S["model_cost_change"] - mref) <= (2 * C * kappa_eps(p["kappa"]) + 16 * EPS) * mref, (at, S["model_cost_change"], mref)
        else:
            ec = float(np.linalg.norm(S["cand"].astype(np.longdouble) - lg["cand"]))
            assert ec <= max(cand_bound, x_bound), (at, "candidate kept", ec, cand_bound)
        if lg.get("solve_end"):
            carry = x_bound


def kappa_eps(kappa):
    return EPS * kappa
