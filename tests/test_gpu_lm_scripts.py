"""-m gpu: the two DEVICE forms of the LM controller on the scripts of lm_script_data.py (so_icp_debug_lm_script: no scan, no map).
  form 0  lm_control_wave, the lane-parallel controller of the persistent solve, run by one wavefront on LDS copies as eval_pass runs it
  form 1  the one-thread controller, by the production lm_step_kernel, one launch per entry
LIMIT: lm_control_wave is force-inlined, so form 0 is a second compilation of its source and not the instance inside solve_kernel;
scripted sums are not injected into the live persistent solve.  What is checked is the source's semantics and its equality with the
one-thread form (whole registrations compare the instances themselves: test_gpu_configs.py).

  * form 0 against form 1, bit for bit: every `more`, every pose handed on, the controller state after EVERY entry, the final state block
    (eval_pose / lm_more only where the one-thread form writes them: the persistent form leaves them alone while a solve continues);
  * the hand-off record of form 0: chunks 0-6 the bits of the pose returned, chunk 7 `more`, all eight carry the tag;
  * device against host and reference: discrete fields equal; whatever no solved step touches bit-equal to the host form; poses and
    continuous state inside the bound of lm_script_run.py (C = 8 x the ratio measured on the CPU: test_lm_scripts_host.py);
  * the context's own registration is not disturbed by a script run."""
import numpy as np
import pytest

import lm_script_data as D
import lm_script_run as R
from helpers import assert_same_bits
from superodom_amd import synth

pytestmark = pytest.mark.gpu
SCRIPTS = {s["name"]: s for s in D.scripts()}
WANT = 0x5A17C0DE0000BEEF


@pytest.fixture(scope="module")
def slam(gpu_slam_factory):
    s = gpu_slam_factory(plane_res=0.2, line_res=0.1)
    yield s
    s.close()


_RUNS = {}


def _run(soicp, slam, s):
    """Both forms of one script (run once, shared by the tests): per form (rows, steps, result)."""
    if s["name"] not in _RUNS:
        entries = [(R.to_sums(soicp, e), e["new_solve"]) for e in s["entries"]]
        out = []
        for form in (0, 1):
            steps, res = slam.debug_lm_script(form, s["x0"], entries, lm_max=s["lm_max"], max_outer=s["max_outer"], outer_iter=s["outer_iter"], want=WANT)
            out.append((steps, res))
        _RUNS[s["name"]] = out
    return _RUNS[s["name"]]


def _rows(steps, logs):
    return [None if lg.get("skipped") else dict(more=st.more, S=R.decode_state(st.state)) for st, lg in zip(steps, logs)]


def _arr(c):
    return np.ctypeslib.as_array(c).copy()


def _check_forms_equal(s, wave, one, logs):
    (sw, rw), (so, ro) = wave, one
    for k, (a, b, lg) in enumerate(zip(sw, so, logs)):
        at = (s["name"], k)
        assert a.more == b.more, at
        assert bytes(a.state) == bytes(b.state), (at, "controller state after the entry")
        if a.more:
            assert bytes(a.pose) == bytes(b.pose), (at, "pose handed on")
        elif not lg.get("skipped"):
            assert R.same_bits(_arr(a.pose), R.decode_state(a.state)["cand"]), (at, "a finished solve hands on the candidate it holds")
    for f in ("state", "T", "T_final", "JtJ", "Jtr", "iterations"):
        assert bytes(getattr(rw, f)) == bytes(getattr(ro, f)), (s["name"], f)
    for f in ("outer_iter", "n_iterations", "reg_done", "done_count"):
        assert getattr(rw, f) == getattr(ro, f), (s["name"], f)
    running = bool(sw[len(sw) - 1].more)
    if not running:   # the one-thread form wrote lm_more = 0 when the solve ended; so did the persistent one
        assert rw.lm_more == ro.lm_more == 0, s["name"]
    else:
        assert ro.lm_more == 1 and bytes(ro.eval_pose) == bytes(sw[len(sw) - 1].pose), s["name"]


def _check_hand_off(s, wave, logs):
    steps, _ = wave
    for k, (st, lg) in enumerate(zip(steps, logs)):
        hand = _arr(st.hand).astype(np.uint64)
        if lg.get("skipped"):
            assert np.all(hand == 0xFFFFFFFF), (s["name"], k, "a skipped entry stores no hand-off")
            continue
        value = hand[:, 0] | (hand[:, 1] << np.uint64(32)); tag = hand[:, 2] | (hand[:, 3] << np.uint64(32))
        assert np.all(tag == np.uint64(WANT)), (s["name"], k, [hex(int(t)) for t in tag])
        assert value[:7].tobytes() == bytes(st.pose), (s["name"], k, "chunks 0-6 are the bits of the pose returned")
        assert int(value[7]) == st.more == lg["more"], (s["name"], k)


def _check_outer(s, res, out):
    assert (res.outer_iter, res.n_iterations, res.reg_done, res.done_count) == (out["outer_iter"], out["n_iterations"], out["reg_done"], out["done_count"]), s["name"]
    assert res.lm_more == out["lm_more"]
    for o in range(16):
        it = res.iterations[o]
        if o not in out["iters"]:
            assert bytes(it) == bytes(len(bytes(it))), (s["name"], o, "a record no solve wrote stays zero")
            continue
        w = out["iters"][o]
        assert (it.lm_iterations, it.num_successful_steps, it.termination) == (w["lm_iterations"], w["num_successful"], w["termination"]), (s["name"], o)
        if w["num_surf"] is not None:
            assert it.num_surf_from_scan == w["num_surf"]
        assert it.initial_cost == w["initial_cost"] and it.final_cost == w["final_cost"]
        assert list(it.reject_hist) == w["hist"][:7] and list(it.obs_hist) == w["hist"][7:], (s["name"], o)
        assert R.same_bits(_arr(it.pose_after), R.decode_state(res.state)["x"]) or o != max(out["iters"])
        assert abs(it.translation_norm - w["translation_norm"]) <= 1e-12 * max(1.0, w["translation_norm"]) + 1e-15
        assert abs(it.rotation_norm - w["rotation_norm"]) <= 1e-10   # (poses within ~1e-13 of the reference's here, and a few eps of its own)
    if out["reg_done"]:
        assert R.same_bits(_arr(res.T_final), _arr(res.T)), s["name"]
        S = R.decode_state(res.state)
        have = S["count"] >= 1
        assert R.same_bits(_arr(res.JtJ).reshape(6, 6), S["H"] if have else np.zeros((6, 6))) and R.same_bits(_arr(res.Jtr), S["g"] if have else np.zeros(6)), s["name"]
    else:
        assert not np.any(_arr(res.T_final)), s["name"]


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_wave_form_equals_one_thread_form_bit_for_bit(soicp, slam, name):
    s = SCRIPTS[name]
    wave, one = _run(soicp, slam, s)
    logs, _ = R.run_ref(s)
    _check_forms_equal(s, wave, one, logs)
    _check_hand_off(s, wave, logs)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", list(SCRIPTS))
def test_device_form_follows_host_and_reference(soicp, slam, name, form):
    s = SCRIPTS[name]
    steps, res = _run(soicp, slam, s)[form]
    logs, out = R.run_ref(s)
    rows = _rows(steps, logs)
    for k, (st, lg) in enumerate(zip(steps, logs)):
        assert st.more == lg["more"], (name, k)
    R.check_against_ref(s, rows, logs)
    _check_outer(s, res, out)
    host, _ = R.run_host(soicp, s)
    accepted = 0
    for k, (d, h, lg) in enumerate(zip(rows, host, logs)):
        if d is None:
            assert h is None; continue
        if lg["decisions"][0] == "begin":
            accepted = 0; solved = False
        accepted += "accepted" in lg["decisions"]
        for f in R.INT_FIELDS + R.EXACT_FIELDS:
            assert R.same_bits_or_nan(d["S"][f], h["S"][f]), (name, k, f, d["S"][f], h["S"][f])
        if accepted == 0:
            assert R.same_bits(d["S"]["inv_radius"], h["S"]["inv_radius"]), (name, k, "radius after rejections only")
        if not solved:   # nothing solved yet in this solve: the whole state is the host's, bit for bit
            if not lg["proposals"]:
                assert d["S"].tobytes() == h["S"].tobytes(), (name, k, "no solved step involved")
        solved = solved or any(p["valid"] for p in lg["proposals"])


def test_recorded_real_problems_on_the_device(soicp, oracle, slam):
    for s, (pose_o, st_o) in D.real_scripts(soicp, oracle):
        wave, one = _run(soicp, slam, s)
        logs, out = R.run_ref(s)
        _check_forms_equal(s, wave, one, logs)
        _check_hand_off(s, wave, logs)
        R.check_against_ref(s, _rows(wave[0], logs), logs)
        S = R.decode_state(wave[1].state)
        assert (S["lm_iterations"], S["num_successful"], S["termination"]) == (st_o.lm_iterations, st_o.num_successful_steps, st_o.termination), s["name"]
        dt, dr = synth.pose_error(S["x"], pose_o)
        assert dt < 1e-9 and dr < 1e-9, (s["name"], dt, dr)


def test_script_run_leaves_the_context_alone(soicp, gpu_slam_factory):
    sc = synth.Scene("tiny")
    a = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_iterations=5)
    a.add_surf_point_cloud(sc.map_points)
    scan, guess = sc.scan(3), sc.guess(3)
    a.register(scan, guess)
    r0, p0, s0 = a.register(scan, guess)   # (the second call: `uncertainty` reports the call before, so both sides follow a registration of this scan)
    for name in ("two_solves_then_one_success", "invalid_last_pivot", "min_radius"):
        s = SCRIPTS[name]
        entries = [(R.to_sums(soicp, e), e["new_solve"]) for e in s["entries"]]
        for form in (0, 1):
            a.debug_lm_script(form, s["x0"], entries, lm_max=s["lm_max"], max_outer=s["max_outer"], outer_iter=s["outer_iter"], want=WANT)
    r1, p1, s1 = a.register(scan, guess)
    assert r0 == r1 == 0 and np.array_equal(p0, p1)
    assert_same_bits(s0, s1, "registration before / after a script run")
    a.close()
