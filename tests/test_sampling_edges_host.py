"""The first stage of a registration on the CPU: the sampling rule (LidarSlam.cpp:346-359) restated in float64 numpy against the oracle's
orc_should_process for every index of every pair of sampling_edge_data.PAIRS, the share partition of knn_query_wave_kernel restated
(query_wave_first, launch_knn_query_waves), the census of every pair -- the guard that a pair takes the path it is named for --, the
host's bound and switch (reg_plan.h through tests/native/reg_plan_host.cpp), and the bucket sizes of binning_edge_data's scan."""
import numpy as np
import pytest

import binning_edge_data as bed
import sampling_edge_data as sed
from superodom_amd import synth
from test_reg_plan_host import rp  # noqa: F401  (the fixture that builds and loads reg_plan.h for the host)

PAIRS = list(sed.PAIRS)


@pytest.mark.parametrize("pair", PAIRS, ids=sed.pair_id)
def test_numpy_rule_is_the_oracles_rule_for_every_index(oracle, pair):
    n, msf = pair
    L = oracle.lib()
    want = np.fromiter((L.orc_should_process(i, n, msf) for i in range(n)), dtype=np.int32, count=n)
    assert set(np.unique(want).tolist()) <= {0, 1}
    got = sed.keeps(n, msf)
    assert np.array_equal(got, want.astype(bool)), (pair, np.nonzero(got != want.astype(bool))[0][:8])
    assert int(got.sum()) == sed.PAIRS[pair]["kept"], (pair, int(got.sum()))


@pytest.mark.parametrize("pair", PAIRS, ids=sed.pair_id)
def test_shares_partition_the_scan(pair):
    n, msf = pair
    per_wave, n_waves = sed.wave_plan(n, msf)
    b = sed.shares(n, msf)
    assert len(b) == n_waves + 1 and b[0] == 0 and b[-1] == n, (pair, b[0], b[-1])
    assert (np.diff(b) >= 0).all(), pair
    # wavefronts beyond n_waves (the grid is rounded up to four per workgroup) own nothing: i_hi = i_lo
    if 0 < msf < n:
        assert n_waves == msf + 1 and per_wave == n / msf
        assert sed.wave_first(msf, n, per_wave) >= n - 1, "the last share is short or empty"
    else:
        assert n_waves == n and per_wave == 1.0 and np.array_equal(b, np.arange(n + 1)), "not sampled: wavefront k owns point k"
    # every kept point lies in exactly one share: searched once
    c = sed.census(n, msf)
    assert len(c["share"]) == c["kept"] and (c["offset"] >= 0).all() and (c["kept_idx"] < b[c["share"] + 1]).all()


@pytest.mark.parametrize("pair", PAIRS, ids=sed.pair_id)
def test_census_is_the_tables(pair):
    n, msf = pair
    want = sed.PAIRS[pair]
    c = sed.census(n, msf)
    print(pair, want["aim"], {k: (v if np.isscalar(v) else len(v)) for k, v in c.items()})
    assert c["kept"] == want["kept"]
    if "late" in want:
        assert len(c["late"]) == want["late"], (pair, "kept points beyond offset 63 of their share", len(c["late"]))
    if "late_at" in want:
        assert set(c["late_offsets"].tolist()) == {want["late_at"]}
        assert (want["late_at"] // 64) + 1 == want["trips"], "the trip of the share loop the pair is named for"
    for k in ("empty", "two", "longest", "trips"):
        if k in want:
            assert c[k] == want[k], (pair, k, c[k], want[k])
    assert c["most"] <= 2, "none, one or two kept points per share"
    if pair in sed.LATE_PAIRS:
        # the late points are second points of their share: the first trip has searched a point, the later trip must load its own
        first_of_share = np.r_[True, np.diff(c["share"]) != 0]
        assert not first_of_share[np.isin(c["kept_idx"], c["late"])].any()


def test_pairs_on_and_under_the_threshold():
    for n, msf in ((1000, 1), (100000, 100)):
        assert msf / n == 0.001 and sed.keeps(n, msf).sum() == msf
    for n, msf in ((1001, 1), (100100, 100)):
        assert msf / n < 0.001 and not sed.keeps(n, msf).any()
    assert np.nonzero(sed.keeps(1000, 1))[0].tolist() == [0]
    assert sed.keeps(50000, 51).sum() == 1 and sed.kept_upper_bound(50000, 51) == 53
    for pair in sed.BIG_PAIRS:
        assert (np.diff(sed.shares(*pair))[:-1] >= 1000).all() and sed.census(*pair)["trips"] == 16


@pytest.mark.parametrize("pair", PAIRS, ids=sed.pair_id)
def test_bound_and_switch_of_the_host_plan(rp, pair):  # noqa: F811
    n, msf = pair
    kept = int(sed.keeps(n, msf).sum())
    bound = rp.rp_kept_upper_bound(msf, n)
    assert bound == sed.kept_upper_bound(n, msf) and kept <= bound, (pair, kept, bound)
    assert bool(rp.rp_query_wave_count_ok(msf, n, sed.QUERY_WAVE_MAX_KEPT)) == sed.takes_query_waves(n, msf)
    want = {(5000, 4095): False, (4097, 4096): False}.get(pair, True)
    assert sed.takes_query_waves(n, msf) == want, (pair, "the sweep the table names")
    if msf == 0:
        assert bound == 2 and sed.wave_plan(n, msf) == (1.0, n), "msf == 0: query waves, one wavefront per point, no cap"


def test_bound_holds_by_brute_force(rp):  # noqa: F811
    worst = -10 ** 9
    for msf in range(1, 80):
        for n in range(msf + 1, 40 * msf + 2):
            kept = int(sed.keeps(n, msf).sum())
            worst = max(worst, kept - msf)
            assert kept <= msf + 2 == rp.rp_kept_upper_bound(msf, n), (n, msf, kept)
    print("max of kept - msf over 1 <= msf < 80, msf < n <= 40 msf + 1:", worst)
    assert worst == 0


def test_scan_of_is_one_pose_and_seeded():
    sc = synth.Scene("small")
    base = sc.scan(0)
    a = sed.scan_of(sc, 27048, 5)
    assert a.shape == (27048, 3) and a.dtype == np.float32 and a.flags.c_contiguous
    assert np.array_equal(a[:len(base)], base) and np.array_equal(a, sed.scan_of(sc, 27048, 5))
    d = np.abs(a[len(base):].astype(np.float64) - base[:27048 - len(base)])
    assert 0 < d.max() < 0.0041, "copies differ from their originals by a few millimetres"
    assert np.array_equal(sed.scan_of(sc, 7, 5), base[:7])


# ------------------------------------------------------------------------------------------------------------------------
# binning
# ------------------------------------------------------------------------------------------------------------------------
def test_chunks_of_a_bucket():
    assert [bed.chunks_of(c) for c in bed.SIZES] == [(0, 1), (0, 1), (1, 0), (1, 0), (1, 0), (1, 1), (1, 1), (2, 0), (2, 0), (2, 1)]
    assert bed.chunks_of(0) == (0, 0) and bed.chunks_of(64 + 17) == (2, 0) and bed.chunks_of(3 * 64) == (3, 0)


def test_bucket_scan_has_the_bucket_sizes_it_is_made_for():
    sc = synth.Scene("small")
    per_size = 30
    scan, owner = bed.bucket_scan(sc.map_points, sc.plane_res, per_size=per_size)
    assert len(scan) == per_size * sum(bed.SIZES) > 4 * 4096 and scan.dtype == np.float32
    sizes = bed.bucket_sizes(scan, sc.plane_res)
    assert np.array_equal(sizes, np.sort(np.repeat(np.array(bed.SIZES), per_size))), np.unique(sizes, return_counts=True)
    # the restated key groups exactly the clusters
    key = bed.grouping_key(scan, sc.plane_res)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    assert len(np.unique(np.stack([inv, owner], 1), axis=0)) == len(bed.SIZES) * per_size
    # well inside one octant: no rounding of the key's arithmetic moves a query
    nc, cell = bed.ked.grid_cells(sc.plane_res)
    u = (scan.astype(np.float64) + 25.0) % 50.0 / (cell / 2)
    f = u - np.floor(u)
    assert f.min() > 0.1 and f.max() < 0.9
    # shuffled: a bucket's queries are spread over the scan, not a run
    assert np.mean(np.diff(owner) != 0) > 0.95
    normal, light = bed.chunk_totals(sizes)
    assert (normal, light) == (11 * per_size, 5 * per_size)
    assert normal + light <= 4096, "the work list fits the sweep's grid"
    # the queries of the scan under the identity: every cube holds map points (the anchors are map points)
    assert bed.ked.cell_counts(sc.map_points, scan).min() > 50


def test_far_cubes_push_the_map_over_the_key_limit():
    pts, cubes = bed.far_cube_points()
    assert len(pts) == 5 * 2100 and len(np.unique(cubes, axis=0)) == 2100 > bed.KEY_SLOT_LIMIT
    assert np.array_equal(np.repeat(cubes, 5, axis=0), bed.ked.cube_of(pts))
    assert ((np.abs(cubes[:, 0]) > 2) | (np.abs(cubes[:, 1]) > 2) | (np.abs(cubes[:, 2]) > 1)).all(), "outside the 5 x 5 x 3 block around the sensor"
    half = np.array(bed.WINDOW) // 2
    assert (np.abs(cubes) <= half).all(), "inside the window"
    # one point per voxel-filter leaf at planeRes 1.0: the map keeps all five
    leaf = np.floor(pts.astype(np.float64) / 1.0).astype(np.int64)
    assert len(np.unique(leaf, axis=0)) == len(pts)
    sc = synth.Scene("small")
    assert np.abs(sc.map_points).max() < 35.0
    assert np.abs(pts).max(axis=1).min() > 35.0 + 50.0, "tens of metres from everything within 35 m of the origin: outside every gate ball"
