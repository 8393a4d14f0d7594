"""-m gpu: what the batch's and the run's correspondence exports share -- one kept-set type, one selection kernel, one host path -- at the two
places neither export's own tests reach: a selection across the two groups of a batch of 70 (its entries lie at h * stride of the kept
arrays and all read ONE scan copy: the scan offset of a table entry differs from its record offset), and both switches on in one
context, where the two kept sets and their two sets of export buffers must not touch each other.  The yardsticks are those of
tests/test_gpu_batch_correspondences.py and tests/test_gpu_sequence_correspondences.py: a twin context that registered the entry
alone, and contexts with one switch on; every comparison is of bytes."""
import numpy as np
import pytest

import batch_correspondences_data as bcd
import sequence_correspondences_data as scd
from helpers import scene_with_oracle
from superodom_amd import synth

pytestmark = pytest.mark.gpu


def _make(make, batch_keep=False, seq_keep=False, keep=False):
    _, slam, _ = scene_with_oracle("tiny", None, make, oracle_too=False, max_iterations=bcd.MAX_OUTER)
    if batch_keep:
        assert slam.keep_batch_correspondences(True) == 0
    if seq_keep:
        assert slam.keep_sequence_correspondences(True) == 0
    if keep:
        assert slam.keep_correspondences(True) == 0
    return slam


def test_a_selection_across_the_groups_of_a_batch_of_70(gpu_slam_factory):
    """hypotheses of both groups of 64, repeated and out of order, through the export (a pose of the caller's per entry) and the sums at
    2 poses: every entry is its twin's to the bit"""
    sc, scan, poses, _ = bcd.batch_inputs("tiny70")
    n, hyp = len(scan), [69, 0, 64, 0, 63]
    slam, twin = _make(gpu_slam_factory, batch_keep=True), _make(gpu_slam_factory, keep=True)
    ok, rcs, out, sts = slam.register_batch(scan, poses)
    assert ok == 70 and (rcs == 0).all()
    at = np.stack([bcd.poses_near(out[h], 2, 700 + 2 * k) for k, h in enumerate(hyp)])  # [entry][pose]: the two entries of hypothesis 0 differ
    assert at[1, 1].tobytes() != at[3, 1].tobytes()
    rec, first, status, infos = slam.batch_correspondences(hyp=hyp, poses=at[:, 1], cap_points=n, cap_records=len(hyp) * n)
    rec0, first0, status0, infos0 = slam.batch_correspondences(hyp=hyp, cap_points=n, cap_records=len(hyp) * n)
    sums = slam.batch_correspondence_sums(at, hyp=hyp)
    assert np.array_equal(first, first0) and status.shape == (len(hyp), n)
    for k, h in enumerate(hyp):
        assert twin.register(scan, poses[h])[0] == 0
        for r, f, s, i, pose in ((rec, first, status, infos, at[k, 1]), (rec0, first0, status0, infos0, None)):
            t_rec, t_status, _, t_info = twin.correspondences(pose=pose, cap=n)
            assert t_info.valid == 1 and t_info.n_accepted > 0
            assert (r[int(f[k]):int(f[k + 1])].tobytes(), s[k].tobytes(), bytes(i[k])) == (t_rec.tobytes(), t_status.tobytes(), bytes(t_info)), (k, h, pose is None)
        t_sums = twin.correspondence_sums(at[k])
        assert [bytes(sums[2 * k + j]) for j in range(2)] == [bytes(t_sums[j]) for j in range(2)], (k, h)
    assert len({status[k].tobytes() for k in (0, 1, 2, 4)}) >= 2, "the hypotheses should differ (tests/test_batch_correspondences_host.py)"
    assert status[1].tobytes() == status[3].tobytes() and bytes(infos[1]) != bytes(infos[3]), "one hypothesis twice, at two poses"
    slam.close(); twin.close()


def test_both_switches_on_in_one_context(gpu_slam_factory):
    """a batch, then a run of 3 frames, then the exports and sums of both, the batch's once more behind the run's: each set is what a
    context with that switch alone leaves behind the same calls"""
    sc, scan, poses, _ = bcd.batch_inputs("tiny5")
    _, scans, pose0, deltas, _, _ = scd.run_inputs("tiny")
    scans, deltas = scans[:3], deltas[:3]
    n, B = len(scan), len(poses)

    def calls(slam, batch, run):
        ok, rcs, out, _ = slam.register_batch(scan, poses)
        assert ok == B
        rc, run_poses, _, _, n_done = slam.register_sequence(scans, pose0, deltas)
        assert rc == 0 and n_done == 3
        at_b = np.stack([bcd.poses_near(out[h], 2, 900 + 2 * h) for h in range(B)])
        at_r = np.stack([scd.poses_near(run_poses[k], 2, 950 + 2 * k) for k in range(3)])
        batch_export = lambda: (lambda r, f, s, i: (r.tobytes(), f.tobytes(), s.tobytes(), [bytes(x) for x in i]))(
            *slam.batch_correspondences(hyp=[4, 0, 2], cap_points=n, cap_records=3 * n))
        run_export = lambda: (lambda r, f, s, fs, i: (r.tobytes(), f.tobytes(), s.tobytes(), fs.tobytes(), [bytes(x) for x in i]))(
            *slam.sequence_correspondences(frames=[2, 0, 1]))
        got = {}
        if batch:
            got["batch"] = (batch_export(), bytes(slam.batch_correspondence_sums(at_b[[4, 0, 2]], hyp=[4, 0, 2])))
        if run:
            got["run"] = (run_export(), bytes(slam.sequence_correspondence_sums(at_r[[2, 0, 1]], frames=[2, 0, 1])))
        if batch and run:  # (behind the other set's export and sums)
            assert (batch_export(), bytes(slam.batch_correspondence_sums(at_b[[4, 0, 2]], hyp=[4, 0, 2]))) == got["batch"]
            assert run_export() == got["run"][0]
        return got

    both, only_batch, only_run = (_make(gpu_slam_factory, batch_keep=b, seq_keep=r) for b, r in ((True, True), (True, False), (False, True)))
    got = calls(both, True, True)
    assert got["batch"] == calls(only_batch, True, False)["batch"], "the batch's set, with and without the run's"
    assert got["run"] == calls(only_run, False, True)["run"], "the run's set, with and without the batch's"
    (b_rec, b_first, _, b_infos), _ = got["batch"]
    (r_rec, r_first, _, _, r_infos), _ = got["run"]
    assert len(b_rec) > 0 and len(r_rec) > 0 and b_rec != r_rec, "two sets of records, and not the same one twice"
    # with its switch off a context exports nothing of that kind, whatever the other switch kept
    assert all(i.valid == 0 for i in only_batch.sequence_correspondences(n_sel=3)[4])
    assert all(i.valid == 0 for i in only_run.batch_correspondences(n_sel=B, cap_points=n, cap_records=0)[3])
    for c in (both, only_batch, only_run):
        c.close()
