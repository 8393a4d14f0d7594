"""CPU suite: every data-dependent path of superodom_amd/csrc/deskew_math.h -- the four branches of matrix_to_quat (three of them
written out by hand, not a transcription of the oracle's indexed form), interpolated_pose before the first entry, exactly on an
entry, in the last interval of a 511 / 512 / 513-entry table and beyond it, and both sides of quat_slerp's threshold with both signs
of the dot -- on the header's host build (tests/deskew_host.py) against the C oracle (bit for bit) and scipy (1e-5 m, the bound of
test_oracle_deskew.py).  The census of tests/deskew_data.py says which path every point takes; the tests assert on it, so that a
case cannot quietly stop reaching its branch.  tests/test_gpu_deskew_branches.py runs the same cases through the kernels."""
import numpy as np
import pytest

import deskew_data as dd
import deskew_host

MANY = 1000  # points a case must put into the branch it was built for (of 4096)


def _count(c, mask):
    return int((mask & c.census["finite"]).sum())


@pytest.fixture(scope="module")
def results(oracle):
    """name -> (host build's (records, start, clamped), oracle's, scipy's xyz), each computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            c = dd.branch_case(name)
            cache[name] = (deskew_host.deskew(*c.args), oracle.deskew(*c.args), dd.scipy_deskew(*c.args))
        return cache[name]
    return get


@pytest.mark.parametrize("name", dd.BRANCH_CASES)
def test_host_build_is_the_oracle_bit_for_bit_and_scipy_to_1e_5(results, name):
    c = dd.branch_case(name)
    (got, start, clamped), (want, wstart, wbeyond), ref = results(name)
    finite = c.census["finite"]
    assert np.array_equal(got, want), "records: every byte (x y z of the finite points, and everything that must stay)"
    assert start.tobytes() == wstart.tobytes(), "the sweep-start frame"
    assert clamped == wbeyond == _count(c, c.census["path"] == dd.CLAMPED), "clamped: the finite points at or beyond the last entry"
    assert np.array_equal(got[~finite], c.rec[~finite]) and (len(c.rec) < 50 or (~finite).sum() >= 1), "non-finite points stay"
    assert np.array_equal(got[:, 12:], c.rec[:, 12:]), "only x y z are rewritten"
    err = np.abs(dd.xyz_of(got)[finite].astype(np.float64) - ref[finite]).max() if finite.any() else 0.0
    print(name, "max |host - scipy|", err, "clamped", clamped)
    assert err < 1e-5


@pytest.mark.parametrize("name,branch", [("ext_x180", 1), ("ext_y180", 2), ("ext_z180", 3), ("ext_near_y", 2), ("ext_near_z", 3)])
def test_census_large_extrinsic_puts_every_point_and_the_start_in_its_branch(name, branch):
    q = dd.branch_case(name).census
    n = int(q["finite"].sum())
    assert n > 4000
    assert (q["quat"][q["finite"], 1] == branch).sum() == n >= MANY, "T_l_i * T_original_current"
    assert (q["quat"][q["finite"], 0] == 0).sum() == n and (q["quat"][q["finite"], 2] == 0).sum() == n, "the products around it: trace > 0"
    assert q["start_quat"] == branch, "start * T_i_l in deskew_setup"


@pytest.mark.parametrize("order", dd.DIAG_ORDERS)
def test_census_every_order_of_the_diagonal(order):
    """the branch is picked by two comparisons of diagonal elements; with only axis-aligned extrinsics the smaller two elements tie or
    hang on the motion, and a selection that ignores one of them goes unnoticed"""
    q = dd.branch_case("ext_diag_%d%d%d" % order).census
    n = int(q["finite"].sum())
    assert (q["diag_order"][q["finite"]] == order).all(1).sum() == n > 4000
    assert (q["quat"][q["finite"], 1] == 1 + order[0]).sum() == n and q["start_quat"] == 1 + order[0]


def test_census_125_degrees_about_111_leaves_the_trace_branch():
    c = dd.branch_case("ext_111_125")
    assert _count(c, c.census["quat"][:, 1] != 0) >= MANY and c.census["start_quat"] != 0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_census_fast_spin_covers_the_trace_branch_and_one_other(axis):
    c = dd.branch_case("spin_" + "xyz"[axis])
    b = c.census["quat"][:, 0]
    assert _count(c, b == 0) >= MANY and _count(c, b == 1 + axis) >= MANY and _count(c, (b != 0) & (b != 1 + axis)) == 0
    assert np.allclose(np.abs(np.sum(c.poses[1:, 4:8] * c.poses[:-1, 4:8], 1)), np.cos(0.1)), "neighbours 0.2 rad apart"


def test_census_interpolated_pose_paths():
    for name in ("exact_vio", "exact_imu"):
        c = dd.branch_case(name)
        assert _count(c, c.census["exact"]) >= 500 and _count(c, (c.census["path"] == dd.INTERIOR) & ~c.census["exact"]) >= MANY
        assert c.census["start_path"] == dd.INTERIOR and (c.poses[:, 0] == c.t0).sum() == 1, "the sweep start sits on an entry too"
    c = dd.branch_case("late")
    assert _count(c, c.census["path"] == dd.BEFORE) >= 500 and c.census["start_path"] == dd.BEFORE
    assert _count(c, c.census["path"] == dd.INTERIOR) >= MANY and _count(c, c.census["path"] == dd.CLAMPED) == 0
    c = dd.branch_case("late_short")
    assert c.census["start_path"] == dd.BEFORE and all(_count(c, c.census["path"] == p) >= 500 for p in (dd.BEFORE, dd.INTERIOR, dd.CLAMPED))


@pytest.mark.parametrize("n", [511, 512, 513])
def test_census_table_edge_reads_the_last_entry(n):
    """kDeskewLdsPoses = 512: 511 and 512 entries go through LDS, 513 through global memory; in each the last points have the last
    entry as "after", and the tail cases read it through the clamp"""
    c = dd.branch_case(f"edge{n}")
    assert len(c.poses) == n and _count(c, c.census["path"] != dd.INTERIOR) == 0
    assert c.census["after"][c.census["finite"]].max() == n - 1 and _count(c, c.census["after"] == n - 1) >= 3
    assert _count(c, c.census["after"] <= 12) >= 3, "and the first entries"
    if n > 511:
        t = dd.branch_case(f"tail{n}")
        assert len(t.poses) == n and _count(t, t.census["path"] == dd.CLAMPED) >= MANY and _count(t, t.census["after"] == n - 1) >= 3


def test_census_slerp_threshold_sides_and_signs():
    q = {k: dd.branch_case(f"threshold_{k}") for k in ("lerp", "slerp", "both")}
    inside = {k: c.census["path"] == dd.INTERIOR for k, c in q.items()}
    for k, c in q.items():
        lerp, neg = c.census["lerp"], c.census["neg"]
        assert _count(c, inside[k]) > 4000
        for side in ((lerp,) if k == "lerp" else (~lerp,) if k == "slerp" else (lerp, ~lerp)):
            assert _count(c, inside[k] & side & neg) >= 400 and _count(c, inside[k] & side & ~neg) >= 400, k
    assert _count(q["lerp"], inside["lerp"] & ~q["lerp"].census["lerp"]) == 0, "no slerp-side interval at all"
    assert _count(q["slerp"], q["slerp"].census["lerp"]) == 0
    # the slerp side sits where the issue puts it: 1 - dot = 1.25e-15 between neighbours 1e-7 rad apart, 5.6 eps below 1
    p = q["slerp"].poses
    d = np.abs(np.sum(p[1:, 4:8] * p[:-1, 4:8], 1))
    assert (1 - d > 4 * 2.220446049250313e-16).all() and (1 - d < 2e-15).all()


@pytest.mark.parametrize("n", dd.CLAMP_SIZES)
def test_census_clamp_counts(n):
    c = dd.branch_case(f"clamp{n}")
    assert len(c.rec) == n
    want = _count(c, c.census["path"] == dd.CLAMPED)
    assert (want == 0) if n == 1 else (0 < want < n), "part of the sweep lies beyond the buffer (the one point of n = 1 is the sweep start)"
    assert _count(c, (c.census["path"] == dd.INTERIOR) & ~c.census["lerp"]) == 0, "no slerp-side interval: the device must give every bit"
    if n <= 63:
        g = dd.branch_case(f"gone{n}")
        assert _count(g, g.census["path"] == dd.CLAMPED) == int(g.census["finite"].sum()) >= 1, "every finite point is clamped"


def test_a_table_whose_times_do_not_increase_is_refused():
    c = dd.branch_case("late")
    same = c.poses.copy(); same[5, 0] = same[4, 0]
    for poses in (c.poses[::-1], same):
        with pytest.raises(ValueError, match="increase strictly"):
            deskew_host.deskew(c.rec, c.time_off, c.t0, poses, c.imu, c.T_i_l)
