"""The shared definitions of "the same registration" (tests/helpers.py: stats_bits / assert_same_bits, assert_follows_oracle) on
hand-built statistics, without a device: every field of the set is perturbed by one unit or one ulp and must be caught BY NAME, must
pass when it is omitted, and the fields outside the set must not matter.  A later edit that drops a field from a set fails here."""
import pickle

import numpy as np
import pytest

import oracle_py
from helpers import (ITER_FIELDS, STATS_FIELDS, assert_follows_oracle, assert_rank_follows_single, assert_same_bits, bits_field,
                     stats_bits, stats_of)
from superodom_amd import binding, synth

N_IT = 3
ORACLE_FIELDS = ("lm_iterations", "num_successful_steps", "termination", "num_surf", "reject_hist", "obs_hist", "final_cost")


def _fill(obj, rng):
    """every field of a ctypes structure to a value of its own"""
    for name, _ in obj._fields_:
        v = getattr(obj, name)
        if isinstance(v, int):
            setattr(obj, name, int(rng.integers(1, 1000)))
        elif isinstance(v, float):
            setattr(obj, name, float(rng.random() + 0.5))
        elif hasattr(v, "_fields_"):
            _fill(v, rng)
        elif hasattr(v[0], "_fields_"):
            for e in v:
                _fill(e, rng)
        else:
            for k in range(len(v)):
                v[k] = int(rng.integers(1, 1000)) if isinstance(v[k], int) else float(rng.random() + 0.5)


def _product_stats():
    st = binding.Stats()
    _fill(st, np.random.default_rng(7))
    st.n_iterations = N_IT
    return st


def _oracle_stats_like(st):
    ost = oracle_py.Stats()
    _fill(ost, np.random.default_rng(8))
    ost.n_iterations = st.n_iterations
    for it in range(st.n_iterations):
        a, b = st.iterations[it], ost.iters[it]
        b.lm_iterations, b.num_successful_steps, b.termination, b.num_surf = a.lm_iterations, a.num_successful_steps, a.termination, a.num_surf_from_scan
        b.final_cost = a.final_cost
        b.reject_hist[:] = list(a.reject_hist); b.obs_hist[:] = list(a.obs_hist)
    return ost


def _perturbations(obj, name):
    """(element index or None, function that moves that element of the field by one unit / one ulp) for every element of the field"""
    v = getattr(obj, name)
    if isinstance(v, int):
        yield None, lambda o: setattr(o, name, getattr(o, name) + 1)
    elif isinstance(v, float):
        yield None, lambda o: setattr(o, name, float(np.nextafter(getattr(o, name), np.inf)))
    else:
        for k in range(len(v)):
            def bump(o, k=k):
                a = getattr(o, name)
                a[k] = a[k] + 1 if isinstance(a[k], int) else float(np.nextafter(a[k], np.inf))
            yield k, bump


def _copy(st):
    return type(st).from_buffer_copy(st)


def test_the_set_is_the_one_the_suite_was_promised():
    assert set(ITER_FIELDS) == {"lm_iterations", "num_successful_steps", "termination", "num_surf_from_scan", "reject_hist", "obs_hist",
                                "initial_cost", "final_cost", "pose_after", "translation_norm", "rotation_norm"}
    assert set(STATS_FIELDS) >= {"JtJ", "Jtr", "uncertainty", "pos_in_localmap", "laser_cloud_surf_from_map_num", "laser_cloud_corner_from_map_num",
                                 "laser_cloud_surf_stack_num", "laser_cloud_corner_stack_num", "startup_count"}
    assert not {"time_elapsed_ms", "flags", "prediction_source"} & (set(ITER_FIELDS) | set(STATS_FIELDS))


@pytest.mark.parametrize("field", ("n_iterations",) + ITER_FIELDS + STATS_FIELDS)
def test_assert_same_bits_catches_one_unit_or_one_ulp_in_every_field(field):
    st = _product_stats()
    assert_same_bits(st, _copy(st), "copy")
    per_iteration = field in ITER_FIELDS
    for it in (range(N_IT) if per_iteration else [None]):
        owner = (lambda o: o.iterations[it]) if per_iteration else (lambda o: o)
        for k, bump in _perturbations(owner(st), field):
            other = _copy(st)
            bump(owner(other))
            with pytest.raises(AssertionError) as e:
                assert_same_bits(st, other, "tag-7")
            msg = str(e.value)
            assert "tag-7" in msg and f": {field} differs" in msg, (field, it, k, msg)
            if per_iteration:
                assert f"at iteration {it}" in msg, msg
            with pytest.raises(AssertionError):  # ... also as what a worker process sends
                assert_same_bits(pickle.loads(pickle.dumps(stats_bits(st))), stats_bits(other), "tag-7")
            if field != "n_iterations":
                assert_same_bits(st, other, "omitted", omit=(field,))
                assert_same_bits(stats_bits(st), stats_bits(other), "omitted", omit=(field,))
                with pytest.raises(AssertionError):
                    assert_same_bits(st, other, "another field omitted", omit=("Jtr" if field != "Jtr" else "JtJ",))


def test_assert_same_bits_leaves_out_what_describes_the_path_and_what_lies_beyond_n_iterations():
    st = _product_stats()
    other = _copy(st)
    other.time_elapsed_ms += 1.0; other.flags ^= binding.FLAG_CHAINED | binding.FLAG_STAGED_SCAN; other.prediction_source += 1
    other.iterations[N_IT].lm_iterations += 1  # (an outer iteration that did not run)
    assert_same_bits(st, other, "path fields")
    assert stats_bits(st) == stats_bits(other) and hash(stats_bits(st)) == hash(stats_bits(other))
    with pytest.raises(AssertionError, match="names no field"):
        stats_bits(st, omit=("final_cots",))


def test_stats_of_is_what_the_rank_processes_send():
    st = _product_stats()
    pose = synth.perturb_pose(np.array([1.0, 2.0, 3.0, 0, 0, 0, 1.0]), 3, 0.1, 1.0)
    a = pickle.loads(pickle.dumps(stats_of((0, pose, st))))
    assert a[0] == 0 and a[1] == pose.tolist() and a[2] == st.flags and a[3] == stats_bits(st)
    assert bits_field(a[3], "n_iterations") == N_IT and bits_field(a[3], "termination", 1) == st.iterations[1].termination
    assert_rank_follows_single(a, a, "itself")
    # a rank's float sums may differ in the last bits, its counts may not, and its pose is held to 1e-9
    other = _copy(st)
    other.iterations[0].final_cost = float(np.nextafter(other.iterations[0].final_cost, 0)); other.JtJ[3] += 1e-9
    assert_rank_follows_single(stats_of((0, pose, other)), a, "another summation tree")
    other.iterations[2].obs_hist[4] += 1
    with pytest.raises(AssertionError, match="obs_hist differs at iteration 2"):
        assert_rank_follows_single(stats_of((0, pose, other)), a, "a count")
    moved = pose.copy(); moved[0] += 2e-9
    with pytest.raises(AssertionError):
        assert_rank_follows_single(stats_of((0, moved, st)), a, "pose")
    with pytest.raises(AssertionError):
        assert_rank_follows_single(stats_of((1, pose, st)), a, "status")


@pytest.mark.parametrize("field", ("n_iterations",) + ORACLE_FIELDS[:-1])
def test_assert_follows_oracle_catches_every_count_and_every_bin(field):
    st = _product_stats()
    ost = _oracle_stats_like(st)
    assert_follows_oracle(st, ost, "equal")
    for it in (range(N_IT) if field != "n_iterations" else [None]):
        owner = (lambda o: o.iters[it]) if field != "n_iterations" else (lambda o: o)
        for k, bump in _perturbations(owner(ost), field):
            other = _copy(ost)
            bump(owner(other))
            with pytest.raises(AssertionError) as e:
                assert_follows_oracle(st, other, "tag-9")
            msg = str(e.value)
            assert "tag-9" in msg and f": {field} differs" in msg, (field, it, k, msg)
            if field != "n_iterations":
                assert f"at iteration {it}" in msg, msg
                assert_follows_oracle(st, other, "omitted", omit=(field,))
                assert_follows_oracle(ost, other, "oracle against oracle, omitted", omit=(field,))
                with pytest.raises(AssertionError):
                    assert_follows_oracle(ost, other, "oracle against oracle")


def test_assert_follows_oracle_holds_the_cost_to_1e_9_relative_and_nothing_else_of_the_floats():
    st = _product_stats()
    ost = _oracle_stats_like(st)
    for it in range(N_IT):
        for cost in (0.75, 4.0e5):  # (relative to max(1, |cost|))
            st.iterations[it].final_cost = cost
            for rel, caught in ((2e-9, True), (-2e-9, True), (5e-10, False), (-5e-10, False)):
                other = _copy(ost)
                other.iters[it].final_cost = cost + rel * max(1.0, cost)
                if caught:
                    with pytest.raises(AssertionError, match=f"final_cost differs at iteration {it}"):
                        assert_follows_oracle(st, other, "cost")
                    assert_follows_oracle(st, other, "cost", omit=("final_cost",))
                    assert_follows_oracle(st, other, "cost", cost_rtol=1e-8)
                else:
                    assert_follows_oracle(st, other, "cost")
            ost.iters[it].final_cost = cost
    ost.iters[0].initial_cost += 1.0; ost.JtJ[0] += 1.0; ost.surf_from_map_num += 1  # (not part of this comparison)
    assert_follows_oracle(st, ost, "other floats")
    with pytest.raises(AssertionError, match="names no field"):
        assert_follows_oracle(st, ost, "typo", omit=("num_surf_from_scan",))


def test_assert_follows_oracle_holds_the_pose_to_the_bound_of_record_and_then_to_1e_8():
    st = _product_stats()
    ost = _oracle_stats_like(st)
    pose = np.array([1.0, 2.0, 3.0, 0, 0, 0, 1.0])
    for d, tol, caught in ((5e-9, 1e-8, False), (2e-8, 1e-8, True), (2e-8, 1e-6, False), (2e-6, 1e-6, True), (2e-4, 1.0, True)):
        moved = pose.copy(); moved[1] += d
        turned = pose.copy(); turned[3:] = synth.quat_from_rotvec(np.array([0.0, d, 0.0]))
        for p in (moved, turned):
            if caught:
                with pytest.raises(AssertionError, match="pose parity violated" if d > 1e-4 else "near machine agreement"):
                    assert_follows_oracle(st, ost, "pose", pose=p, opose=pose, pose_tol=tol)
            else:
                assert_follows_oracle(st, ost, "pose", pose=p, opose=pose, pose_tol=tol)
