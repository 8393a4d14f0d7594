"""-m gpu: one pose prior per hypothesis of a batch (so_icp_set_batch_priors), inside the batched persistent solve.  The contract --
hypothesis h is so_icp_set_pose_prior(P_h) + so_icp_register_dev from poses_in[h], bit for bit -- on the batched kernels (workgroups per
hypothesis that do not divide the grid, more than one group of 64, a sub-sampled scan) and on every other path a batch can take; nothing
changes where there is no prior; hypotheses that fail, an empty map, an empty scan; the state rules; and the last outer iteration of a
hypothesis against so_icp_correspondence_sums + so_icp_pose_prior_sums.  Inputs: tests/batch_priors_data.py, which the CPU suite shows to
be discriminating."""
import ctypes as C

import numpy as np
import pytest

import batch_priors_data as bpd
import pose_prior_ref as ppr
from helpers import assert_same_bits, scene_with_oracle, stats_bits
from superodom_amd import synth

pytestmark = pytest.mark.gpu
IU = np.triu_indices(6)
OMIT = ("uncertainty",)  # (from the call before: the single registrations advance it, the batch does not)


def _make(make, scene, sub=None, keep=False):
    _, slam, _ = scene_with_oracle(scene, None, make, oracle_too=False, max_iterations=bpd.MAX_OUTER)
    if sub:
        slam.set_max_surface_features(sub)
    if keep:
        assert slam.keep_correspondences(True) == 0
    return slam


def _single(slam, P, d, n, guess):
    """the registration the contract names: so_icp_set_pose_prior(P_h) + so_icp_register_dev, plain where the hypothesis has no prior"""
    if P is not None:
        slam.set_pose_prior(P)
    return slam.register_dev(d, n, guess)


def _check_against_singles(soicp, slam, d, n, poses, priors, modes, rcs, out, sts, tag):
    outer = []
    for h in range(len(poses)):
        P = bpd.hypothesis_prior(priors, modes, h, poses[h])
        rc, ph, sh = _single(slam, P, d, n, poses[h])
        assert rc == int(rcs[h]), (tag, h, rc, int(rcs[h]))
        assert np.array_equal(ph, out[h]), (tag, h)
        assert_same_bits(sts[h], sh, (tag, h), omit=OMIT)
        has = modes[h] != bpd.NONE
        assert bool(sts[h].flags & soicp.FLAG_POSE_PRIOR) == has == bool(sh.flags & soicp.FLAG_POSE_PRIOR), (tag, h)
        assert sts[h].prediction_source == sh.prediction_source == (1 if has else 0), (tag, h)
        outer.append(sh.n_iterations)
    return outer


# the batch of ("small9", kind) on the default path: the reference of the path tests, computed once
_default = {}


@pytest.fixture(scope="module")
def default_small9(gpu_slam_factory):
    def get(kind):
        if kind not in _default:
            sc, scan, poses, priors, modes, sub = bpd.batch_inputs("small9", kind)
            slam = _make(gpu_slam_factory, "small", sub)
            slam.set_batch_priors(priors, modes)
            ok, rcs, out, sts = slam.register_batch(scan, poses)
            assert ok == len(poses)
            _default[kind] = (scan, poses, priors, modes, sub, out.copy(), [stats_bits(s) for s in sts], [s.flags for s in sts])
            slam.close()
        return _default[kind]
    yield get
    _default.clear()


# ---- 1. the contract ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", bpd.U_KINDS)
@pytest.mark.parametrize("case", list(bpd.CASES))
def test_every_hypothesis_equals_its_single_registration_with_its_prior(soicp, gpu_slam_factory, case, kind):
    sc, scan, poses, priors, modes, sub = bpd.batch_inputs(case, kind)
    slam = _make(gpu_slam_factory, bpd.CASES[case][0], sub)
    d, n = slam.upload_scan(scan)
    slam.set_batch_priors(priors, modes)
    ok, rcs, out, sts = slam.register_batch(None, poses, d_scan=d, n=n)
    assert ok == len(poses) and (rcs == 0).all()
    outer = _check_against_singles(soicp, slam, d, n, poses, priors, modes, rcs, out, sts, (case, kind))
    print(case, kind, "outer iterations", outer)
    if case == "tiny70":
        assert len(set(outer)) >= 2, "the hypotheses should leave the rounds at different times (stale chained rounds)"
    slam.close()


# ---- 2. other paths, same bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", bpd.U_KINDS)
@pytest.mark.parametrize("env", [{"SOICP_BATCH_MODE": "lanes"}, {"SOICP_BATCH_MODE": "one_per_cu"}, {"SOICP_BATCH_CHAIN": "0"}])
def test_the_other_paths_of_a_batch_give_the_same_bits(soicp, gpu_slam_factory, monkeypatch, default_small9, env, kind):
    scan, poses, priors, modes, sub, out, bits, flags = default_small9(kind)
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # read by so_icp_create
    alt = _make(gpu_slam_factory, "small", sub)
    alt.set_batch_priors(priors, modes)
    ok, rcs, out2, sts2 = alt.register_batch(scan, poses)
    assert ok == len(poses) and np.array_equal(out2, out)
    for h in range(len(poses)):
        assert_same_bits(bits[h], sts2[h], (env, kind, h))
        assert bool(sts2[h].flags & soicp.FLAG_POSE_PRIOR) == (modes[h] != bpd.NONE) and sts2[h].prediction_source == (modes[h] != bpd.NONE), (env, h)
    alt.close()


def test_a_resident_scan_and_a_second_batch_give_the_same_bits(soicp, gpu_slam_factory, default_small9):
    scan, poses, priors, modes, sub, out, bits, flags = default_small9("dense")
    slam = _make(gpu_slam_factory, "small", sub)
    d, n = slam.upload_scan(scan)
    for round_ in ("resident", "second batch: chained by the survivor counts of the first"):
        slam.set_batch_priors(priors, modes)
        ok, rcs, out2, sts2 = slam.register_batch(None, poses, d_scan=d, n=n)
        assert ok == len(poses) and np.array_equal(out2, out), round_
        for h in range(len(poses)):
            assert_same_bits(bits[h], sts2[h], (round_, h))
            assert sts2[h].flags == flags[h], (round_, h)
    slam.close()


# ---- 3. nothing changes where there is no prior -------------------------------------------------------------------------------------------
def test_nothing_changes_where_there_is_no_prior(soicp, gpu_slam_factory):
    sc, scan, poses, priors, modes, sub = bpd.batch_inputs("small9", "dense")
    slam = _make(gpu_slam_factory, "small", sub)
    d, n = slam.upload_scan(scan)
    B = len(poses)
    ok, rcs0, out0, sts0 = slam.register_batch(None, poses, d_scan=d, n=n)
    assert ok == B and all(s.prediction_source == 0 and not (s.flags & soicp.FLAG_POSE_PRIOR) for s in sts0)
    # all NONE (every word of every prior poisoned): the batch without priors, flags included
    nan_all = soicp.PosePrior.from_buffer_copy(np.full(55, np.nan).tobytes())
    slam.set_batch_priors([nan_all] * B, [bpd.NONE] * B)
    ok, rcs, out, sts = slam.register_batch(None, poses, d_scan=d, n=n)
    assert ok == B and np.array_equal(out, out0)
    for h in range(B):
        assert_same_bits(sts[h], sts0[h], ("all NONE", h))
        assert sts[h].flags == sts0[h].flags and sts[h].prediction_source == 0, h
    # U = 0 on every hypothesis: a prior that adds nothing
    zero = [soicp.pose_prior(sc.gt_pose(bpd.SCAN_ID), np.zeros((6, 6)), ppr.REFERENCE_FLOOR, ppr.REFERENCE_FRACTION)] * B
    slam.set_batch_priors(zero)
    ok, rcs, out, sts = slam.register_batch(None, poses, d_scan=d, n=n)
    assert ok == B and np.array_equal(out, out0)
    for h in range(B):
        assert_same_bits(sts[h], sts0[h], ("U = 0", h))
        assert sts[h].flags == sts0[h].flags | soicp.FLAG_POSE_PRIOR and sts[h].prediction_source == 1, h
    # a mixed batch: its NONE hypotheses are the plain hypotheses, and the plain single registrations
    slam.set_batch_priors(priors, modes)
    ok, rcs, out, sts = slam.register_batch(None, poses, d_scan=d, n=n)
    assert ok == B
    none = [h for h in range(B) if modes[h] == bpd.NONE]
    assert len(none) >= 2
    for h in range(B):
        if h in none:
            assert np.array_equal(out[h], out0[h])
            assert_same_bits(sts[h], sts0[h], ("mixed, NONE", h))
            assert sts[h].flags == sts0[h].flags and sts[h].prediction_source == 0, h
            rc, ph, sh = slam.register_dev(d, n, poses[h])
            assert rc == 0 and np.array_equal(ph, out[h])
            assert_same_bits(sts[h], sh, ("mixed, NONE, single", h), omit=OMIT)
        else:
            assert not np.array_equal(out[h], out0[h]), (h, "the prior does not move the result")
    slam.close()


# ---- 4. degenerate members ----------------------------------------------------------------------------------------------------------------
def test_hypotheses_that_fail_an_empty_map_and_an_empty_scan(soicp, gpu_slam_factory):
    """test_gpu_configs.py::test_batch_with_hypotheses_that_fail_and_degenerate_inputs' guesses, the far and the turned ones with priors"""
    slam = _make(gpu_slam_factory, "small")
    sc = synth.Scene("small")
    i = 4
    scan = np.ascontiguousarray(sc.scan(i), np.float32)
    gt = sc.gt_pose(i)
    far = gt.copy(); far[2] += 8.0
    turned = gt.copy()
    turned[3:] = synth.quat_mul(gt[3:], synth.quat_from_rotvec(np.array([0.0, 0.0, np.pi / 2])))
    near = [synth.perturb_pose(gt, 8100 + h, 0.1, 1.0) for h in range(3)]
    poses = np.stack([near[0], far, near[1], turned, near[0], far, near[2]])
    modes = [bpd.GIVEN, bpd.AT_GUESS, bpd.NONE, bpd.GIVEN, bpd.AT_GUESS, bpd.GIVEN, bpd.AT_GUESS]
    for kind in bpd.U_KINDS:
        priors = bpd.priors_for(sc, len(poses), kind, modes, i=i)
        d, n = slam.upload_scan(scan)
        slam.set_batch_priors(priors, modes)
        ok, rcs, out, sts = slam.register_batch(None, poses, d_scan=d, n=n)
        _check_against_singles(soicp, slam, d, n, poses, priors, modes, rcs, out, sts, ("mixed batch", kind))
        assert ok == int((rcs == 0).sum())
        print(kind, "rc", [int(r) for r in rcs], "terminations", [[s.iterations[k].termination for k in range(s.n_iterations)] for s in sts])
        assert sts[1].iterations[0].num_surf_from_scan < sts[0].iterations[0].num_surf_from_scan / 2, "far fewer matches from 8 m above (planes only)"
    # an empty scan: the hypotheses as concurrent registrations on worker contexts
    none = np.zeros((0, 3), np.float32)
    slam.set_batch_priors(priors[:3], modes[:3])
    ok, rcs, out, sts = slam.register_batch(none, poses[:3])
    singles = []
    for h in range(3):
        P = bpd.hypothesis_prior(priors, modes, h, poses[h])
        if P is not None:
            slam.set_pose_prior(P)
        singles.append(slam.register(none, poses[h]))
    assert [int(r) for r in rcs] == [r[0] for r in singles] and ok == int((rcs == 0).sum())
    for h in range(3):
        assert np.array_equal(out[h], singles[h][1]), h
        assert (sts[h].flags & soicp.FLAG_POSE_PRIOR) == (singles[h][2].flags & soicp.FLAG_POSE_PRIOR), h
    rc, _, st = slam.register(scan, poses[0])
    assert rc == 0 and not (st.flags & soicp.FLAG_POSE_PRIOR), "the empty-scan batch consumed its priors"
    slam.close()
    # an empty map: every hypothesis finds too little map, the priors are consumed, no prior flag is set
    empty = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=bpd.MAX_OUTER)
    empty.set_batch_priors(priors, modes)
    ok, rcs, out, sts = empty.register_batch(scan, poses)
    assert ok == 0 and (rcs == soicp.NOT_ENOUGH_MAP_FEATURES).all() and np.array_equal(out, poses)
    assert all(not (s.flags & soicp.FLAG_POSE_PRIOR) and s.prediction_source == 0 for s in sts)
    assert empty.register(scan, poses[0])[0] == soicp.NOT_ENOUGH_MAP_FEATURES, "the priors were consumed: so_icp_register is not refused"
    empty.close()


# ---- 5. state rules -----------------------------------------------------------------------------------------------------------------------
def test_one_shot_count_withdrawal_and_refusals(soicp, gpu_slam_factory):
    sc, scan, poses, priors, modes, sub = bpd.batch_inputs("tiny5", "dense")
    poses, modes = poses[:3], [bpd.GIVEN, bpd.AT_GUESS, bpd.AT_GUESS]
    given = bpd.hypothesis_prior(priors, [bpd.AT_GUESS] * 3, 0, synth.perturb_pose(sc.gt_pose(bpd.SCAN_ID), 900, 0.02, 0.2))  # (a finite T_meas)
    priors = [given, priors[1], priors[2]]
    slam = _make(gpu_slam_factory, "tiny", keep=True)
    guess = poses[0]
    deltas = np.zeros((2, 7)); deltas[:, 6] = 1.0

    def has_prior(res):
        return [bool(st.flags & soicp.FLAG_POSE_PRIOR) for st in res[3]]
    # one-shot: the batch after a batch with priors carries none
    slam.set_batch_priors(priors, modes)
    assert has_prior(slam.register_batch(scan, poses)) == [True, True, True]
    assert has_prior(slam.register_batch(scan, poses)) == [False, False, False]
    # NULL modes: all GIVEN
    slam.set_batch_priors([given] * 3)
    assert has_prior(slam.register_batch(scan, poses)) == [True, True, True]
    # a batch of another size is refused before it touches anything and leaves them pending
    slam.set_batch_priors(priors, modes)
    with pytest.raises(soicp.SoIcpError, match="so_icp error -1: .*n_hyp differs"):
        slam.register_batch(scan, poses[:2])
    # ... as do the entries that cannot carry them, and the two other setters
    for call in (lambda: slam.register(scan, guess), lambda: slam.register_dev(*slam.upload_scan(scan), guess),
                 lambda: slam.localization(True, guess, scan, 0.1), lambda: slam.localization_dev(True, guess, *slam.upload_scan(scan), 0.1),
                 lambda: slam.register_sequence([scan, scan], guess, deltas), lambda: slam.localization_sequence([scan, scan], guess, deltas, [0.1, 0.2]),
                 lambda: slam.match(scan, guess), lambda: slam.match_dev(*slam.upload_scan(scan), guess),
                 lambda: slam.set_pose_prior(given), lambda: slam.set_sequence_priors([given, given])):
        with pytest.raises(soicp.SoIcpError, match="so_icp error -5: .*priors of a batch are pending"):
            call()
    assert has_prior(slam.register_batch(scan, poses)) == [True, True, True], "the refused calls left the priors pending"
    assert has_prior(slam.register_batch(scan, poses)) == [False, False, False]
    # withdrawal: n_hyp 0, priors NULL
    for withdraw in (lambda: slam.L.so_icp_set_batch_priors(slam.h, 0, (soicp.PosePrior * 3)(*priors), None), lambda: slam.set_batch_priors(None)):
        slam.set_batch_priors(priors, modes)
        assert withdraw() in (0, None)
        assert slam.register(scan, guess)[0] == 0
        assert has_prior(slam.register_batch(scan, poses)) == [False, False, False]
    # the setter is refused while a single prior or the priors of a run are pending; those stay pending, and the batch refuses them as before
    slam.set_pose_prior(given)
    with pytest.raises(soicp.SoIcpError, match="so_icp error -5: .*pose prior is pending"):
        slam.set_batch_priors(priors, modes)
    with pytest.raises(soicp.SoIcpError, match="so_icp error -5: .*pose prior is pending"):
        slam.register_batch(scan, poses)
    rc, _, st = slam.register(scan, guess)
    assert rc == 0 and (st.flags & soicp.FLAG_POSE_PRIOR)
    slam.set_sequence_priors([given, given])
    with pytest.raises(soicp.SoIcpError, match="so_icp error -5: .*priors of a run are pending"):
        slam.set_batch_priors(priors, modes)
    with pytest.raises(soicp.SoIcpError, match="so_icp error -5: .*priors of a run are pending"):
        slam.register_batch(scan, poses)
    assert [bool(st.flags & soicp.FLAG_POSE_PRIOR) for st in slam.register_sequence([scan, scan], guess, deltas)[3]] == [True, True]
    assert has_prior(slam.register_batch(scan, poses)) == [False, False, False], "the refused setter calls left nothing pending"
    # validation: on the words a mode reads
    arr = lambda ps: (soicp.PosePrior * len(ps))(*ps)
    u8 = lambda ms: (C.c_uint8 * len(ms))(*ms)
    set_raw = lambda ps, ms: slam.L.so_icp_set_batch_priors(slam.h, len(ps), arr(ps), u8(ms) if ms is not None else None)

    def broken(**fields):
        p = soicp.PosePrior.from_buffer_copy(bytes(given))
        for name, (i, v) in fields.items():
            getattr(p, name)[i] = v
        return p
    assert set_raw([given, broken(sqrt_information=(7, float("nan")))], [bpd.GIVEN, bpd.GIVEN]) == -1
    assert set_raw([given, broken(sqrt_information=(9, float("inf")))], [bpd.GIVEN, bpd.AT_GUESS]) == -1
    assert set_raw([given, broken(T_meas=(0, float("nan")))], None) == -1
    zero_q = soicp.PosePrior.from_buffer_copy(bytes(given))
    for i in range(3, 7):
        zero_q.T_meas[i] = 0.0
    assert set_raw([zero_q, given], [bpd.GIVEN, bpd.GIVEN]) == -1 and b"zero norm" in slam.L.so_icp_last_error(slam.h)
    assert set_raw([given, given], [bpd.GIVEN, 3]) == -1
    assert has_prior(slam.register_batch(scan, poses[:2])) == [False, False], "a refused call leaves nothing pending"
    # a refused call leaves what WAS pending
    slam.set_batch_priors(priors, modes)
    assert set_raw([given, given, given], [bpd.GIVEN, 3, bpd.GIVEN]) == -1
    assert has_prior(slam.register_batch(scan, poses)) == [True, True, True]
    # T_meas of an AT_GUESS hypothesis and every word of a NONE hypothesis are not read
    nan_all = soicp.PosePrior.from_buffer_copy(np.full(55, np.nan).tobytes())
    assert set_raw([zero_q, nan_all, broken(T_meas=(0, float("nan")))], [bpd.AT_GUESS, bpd.NONE, bpd.AT_GUESS]) == 0
    assert has_prior(slam.register_batch(scan, poses)) == [True, False, True]
    slam.close()
    # a sharded context
    sharded = gpu_slam_factory(plane_res=sc.plane_res, world_size=2, rank=0)
    assert sharded.L.so_icp_set_batch_priors(sharded.h, 3, arr(priors), None) == -5
    sharded.close()


# Which entry refuses which pending kind, and the whole text it leaves in so_icp_last_error
PENDING_TEXT = {
    "single": "a pose prior is pending (so_icp_set_pose_prior); it goes into so_icp_register(_dev) or so_icp_localization(_dev) -- "
              "withdraw it with so_icp_set_pose_prior(ctx, NULL) first",
    "run": "the priors of a run are pending (so_icp_set_sequence_priors); they go into so_icp_register_sequence or "
           "so_icp_localization_sequence -- withdraw them with so_icp_set_sequence_priors(ctx, 0, NULL, NULL) first",
    "batch": "the priors of a batch are pending (so_icp_set_batch_priors); they go into so_icp_register_batch -- withdraw them with "
             "so_icp_set_batch_priors(ctx, 0, NULL, NULL) first",
}
REFUSED_BY = {
    "single": ("so_icp_register_sequence", "so_icp_localization_sequence", "so_icp_set_sequence_priors", "so_icp_register_batch",
               "so_icp_set_batch_priors", "so_icp_match", "so_icp_match_dev"),
    "run": ("so_icp_register", "so_icp_register_dev", "so_icp_localization", "so_icp_localization_dev", "so_icp_set_pose_prior",
            "so_icp_register_batch", "so_icp_set_batch_priors", "so_icp_match", "so_icp_match_dev"),
    "batch": ("so_icp_register", "so_icp_register_dev", "so_icp_localization", "so_icp_localization_dev", "so_icp_set_pose_prior",
              "so_icp_register_sequence", "so_icp_localization_sequence", "so_icp_set_sequence_priors", "so_icp_match", "so_icp_match_dev"),
}


def test_every_refusal_by_code_and_whole_text_and_the_withdrawal_order(soicp, gpu_slam_factory):
    """Each kind of prior pending in turn: every entry that cannot take it returns -5 with the whole text above and leaves it pending;
    so_icp_set_pose_prior(ctx, NULL) is refused like any other call of it, a withdrawal through one of the two other setters comes before
    the refusal check and touches only its own kind, and a setter call that fails validation inside its list leaves what was pending."""
    sc, scan, poses, priors, _, _ = bpd.batch_inputs("tiny5", "dense")
    poses, guess = poses[:3], poses[0]
    given = bpd.hypothesis_prior(priors, [bpd.AT_GUESS] * 3, 0, synth.perturb_pose(sc.gt_pose(bpd.SCAN_ID), 900, 0.02, 0.2))  # (a finite T_meas)
    slam = _make(gpu_slam_factory, "tiny", keep=True)  # (so_icp_match refuses a context without the switch first)
    d, n = slam.upload_scan(scan)
    deltas = np.zeros((2, 7)); deltas[:, 6] = 1.0
    entries = {
        "so_icp_register": lambda: slam.register(scan, guess), "so_icp_register_dev": lambda: slam.register_dev(d, n, guess),
        "so_icp_localization": lambda: slam.localization(True, guess, scan, 0.1),
        "so_icp_localization_dev": lambda: slam.localization_dev(True, guess, d, n, 0.1),
        "so_icp_set_pose_prior": lambda: slam.set_pose_prior(given),
        "so_icp_register_sequence": lambda: slam.register_sequence([scan, scan], guess, deltas),
        "so_icp_localization_sequence": lambda: slam.localization_sequence([scan, scan], guess, deltas, [0.1, 0.2]),
        "so_icp_set_sequence_priors": lambda: slam.set_sequence_priors([given, given]),
        "so_icp_register_batch": lambda: slam.register_batch(scan, poses), "so_icp_set_batch_priors": lambda: slam.set_batch_priors([given] * 3),
        "so_icp_match": lambda: slam.match(scan, guess), "so_icp_match_dev": lambda: slam.match_dev(d, n, guess),
    }
    assert set(entries) == {e for es in REFUSED_BY.values() for e in es}

    def refused(entry, call, kind):
        with pytest.raises(soicp.SoIcpError) as e:
            call()
        assert str(e.value) == "so_icp error -5: %s: %s" % (entry, PENDING_TEXT[kind]), (kind, entry)
        assert slam.last_error() == "%s: %s" % (entry, PENDING_TEXT[kind]), (kind, entry)
    set_kind = {"single": lambda: slam.set_pose_prior(given), "run": lambda: slam.set_sequence_priors([given, given]),
                "batch": lambda: slam.set_batch_priors([given] * 3)}
    # the entry that takes the kind: every frame / hypothesis of it then carries a prior, and the same call again none
    takes = {"single": lambda: [slam.register(scan, guess)[2]], "run": lambda: slam.register_sequence([scan, scan], guess, deltas)[3],
             "batch": lambda: slam.register_batch(scan, poses)[3]}

    def consumed_by_its_entry(kind, tag):
        for want in (True, False):
            assert [bool(st.flags & soicp.FLAG_POSE_PRIOR) for st in takes[kind]()] == [want] * {"single": 1, "run": 2, "batch": 3}[kind], (kind, tag, want)
    arr = lambda ps: (soicp.PosePrior * len(ps))(*ps)
    nan_u = soicp.PosePrior.from_buffer_copy(bytes(given)); nan_u.sqrt_information[7] = float("nan")
    for kind in ("single", "run", "batch"):
        set_kind[kind]()
        for entry in REFUSED_BY[kind]:
            refused(entry, entries[entry], kind)
        if kind != "single":  # the refusal check of so_icp_set_pose_prior comes before its withdrawal
            refused("so_icp_set_pose_prior", lambda: slam.set_pose_prior(None), kind)
        # n 0 withdraws before any refusal check: SO_ICP_OK while another kind is pending, which stays
        if kind != "run":
            assert slam.L.so_icp_set_sequence_priors(slam.h, 0, None, None) == 0 and slam.L.so_icp_set_sequence_priors(slam.h, 0, arr([given]), None) == 0
        if kind != "batch":
            assert slam.L.so_icp_set_batch_priors(slam.h, 0, None, None) == 0 and slam.L.so_icp_set_batch_priors(slam.h, 2, None, None) == 0
        refused("so_icp_match", entries["so_icp_match"], kind)
        consumed_by_its_entry(kind, "after the refused calls and the withdrawals of the other kinds")
    # a setter call that fails validation half-way through its list leaves what was pending
    for kind, setter in (("run", slam.L.so_icp_set_sequence_priors), ("batch", slam.L.so_icp_set_batch_priors)):
        set_kind[kind]()
        assert setter(slam.h, 3, arr([given, nan_u, given]), None) == -1
        assert slam.last_error() == "so_icp_set_%s_priors: a field of priors[1] is not finite" % {"run": "sequence", "batch": "batch"}[kind]
        consumed_by_its_entry(kind, "after a call that failed validation")
    set_kind["single"]()
    assert slam.L.so_icp_set_pose_prior(slam.h, C.byref(nan_u)) == -1 and slam.last_error() == "so_icp_set_pose_prior: a field of the prior is not finite"
    consumed_by_its_entry("single", "after a call that failed validation")
    # each kind withdrawn by its own setter
    for kind, withdraw in (("single", lambda: slam.set_pose_prior(None)), ("run", lambda: slam.set_sequence_priors(None)), ("batch", lambda: slam.set_batch_priors(None))):
        set_kind[kind]()
        withdraw()
        assert not any(st.flags & soicp.FLAG_POSE_PRIOR for st in takes[kind]()), kind
    slam.close()


# ---- 6. the last outer iteration against a direct evaluation ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", bpd.U_KINDS)
def test_last_outer_iteration_against_correspondence_sums_and_the_host_prior(soicp, gpu_slam_factory, kind):
    """Hypothesis 0 (GIVEN) of "tiny5": a twin context registers it singly with so_icp_keep_correspondences on -- the registration the
    contract (test 1) holds the batch to, and equal to the batch's hypothesis here too.  Its last outer iteration's initial_cost and
    final_cost are the kept set's sums at the pose that iteration started from / ended at, so_icp_pose_prior_sums added on the host:
    the relation test_gpu_pose_prior.py::test_final_normal_equations holds the single registration to."""
    sc, scan, poses, priors, modes, sub = bpd.batch_inputs("tiny5", kind)
    h = 0
    assert modes[h] == bpd.GIVEN
    P = bpd.hypothesis_prior(priors, modes, h, poses[h])
    slam = _make(gpu_slam_factory, "tiny")
    slam.set_batch_priors(priors, modes)
    ok, rcs, out, sts = slam.register_batch(scan, poses)
    assert ok == len(poses)
    slam.close()
    twin = _make(gpu_slam_factory, "tiny", keep=True)
    twin.set_pose_prior(P)
    rc, pose, st = twin.register(scan, poses[h])
    assert rc == 0 and np.array_equal(pose, out[h])
    assert_same_bits(sts[h], st, ("batch against the twin", kind), omit=OMIT)
    last = st.iterations[st.n_iterations - 1]
    x1 = np.array(last.pose_after)
    x0 = np.array(st.iterations[st.n_iterations - 2].pose_after) if st.n_iterations >= 2 else np.asarray(poses[h], float)
    at_start, at_end = twin.correspondence_sums(np.stack([x0, x1]))
    assert at_start.count == at_end.count == last.num_surf_from_scan
    for name, planes, x, got in (("initial_cost", at_start, x0, last.initial_cost), ("final_cost", at_end, x1, last.final_cost)):
        prior_cost = ppr.host_prior_sums(P, x, planes.count).cost
        print(f"{kind} {name}: registration {got!r}, planes {planes.cost!r} + prior {prior_cost!r}")
        assert prior_cost > 0
        assert abs((got - prior_cost) - planes.cost) <= 1e-9 * max(1.0, abs(planes.cost)), (name, got, prior_cost, planes.cost)
    both = ppr.host_prior_sums(P, x1, at_end.count)
    for got, want in ((np.array(st.JtJ).reshape(6, 6)[IU] - np.array(both.JtJ[:]), np.array(at_end.JtJ[:])), (np.array(st.Jtr) - np.array(both.Jtr[:]), np.array(at_end.Jtr[:]))):
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max()), (got, want)
    twin.close()
