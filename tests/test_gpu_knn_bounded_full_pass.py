"""-m gpu: the FULL pass of the chunked sweep bounded by the near pass's exact 5th distance (knn_plane_kernel, SO_KNN_BOUNDED_FULL).

knn_second_pass_data.bounded(): one chunk per site -- ordinary (40 queries), split (24) and light (12) -- built relative to the faces of
its near block (sites a .. g, see the module).  One registration with
max_iterations = 1 under the identity; status bytes and neighbour lists of EVERY query are compared bit for bit with the numpy brute
force and with the oracle, with SOICP_KNN_PACK 0 and 1, on the production and the instrumented instantiation; one case goes through
so_icp_register_sequence (the chained BEGIN launch).  So that a pass cannot hide a failure: every site's preconditions are asserted from
the brute force (no site is skipped), and the instrumented run's counters must show that second passes ran.
Site h (pending lanes of one chunk in two cubes) needs a scan binned ahead under another pose: the last test.

`knn_fallback_lanes` is compared with the figure the same run gives on a library built with -DSO_KNN_BOUNDED_FULL=0 (recorded below from
such a run: a test cannot build a second library in seconds): the bound must not send more lanes to the exact scan."""
import numpy as np
import pytest

import knn_edge_data as ked
import knn_second_pass_data as spd
from test_gpu_knn_edges import (ABLATE_STATS_ONLY, IDENTITY, JUDGED, _check_lists, _expect_status, _export_index, _product, _register, _scan_of)

pytestmark = pytest.mark.gpu

# knn_fallback_lanes of test_sweep's instrumented run on a library built with SOICP_EXTRA_CXXFLAGS=-DSO_KNN_BOUNDED_FULL=0, per SOICP_KNN_PACK
# (profiles/knn_second_pass/README.md, "Tests")
FALLBACK_LANES_UNBOUNDED = {"1": 0, "0": 0}

_state = {}


def _setup(oracle, make):
    if not _state:
        fam = spd.bounded()
        slam = _product(make, fam)
        exp = slam.export_map()
        slam.close()
        order = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
        assert np.array_equal(order(exp).view(np.uint32), order(fam.map_points).view(np.uint32)), "the map IS the generated one"
        om = oracle.OracleMap(plane_res=fam.plane_res)
        om.add_surf(exp, raw=True)
        assert np.array_equal(om.export(), exp)
        scan = _scan_of(fam)
        ref = ked.brute_knn(exp, scan, n_tail=2)
        orc, _, _, corrs = om.register(scan, IDENTITY, oracle.default_config(max_iterations=1), want_corrs=True)
        assert orc == 0
        _state.update(fam=fam, exp=exp, om=om, scan=scan, ref=ref, corrs=corrs, n_checked=spd.check_sites(fam, exp, ref))
    s = _state
    return s["fam"], s["exp"], s["om"], s["scan"], s["ref"], s["corrs"]


def _prof(make, monkeypatch, fam, scan):
    monkeypatch.setenv("SOICP_ABLATE", ABLATE_STATS_ONLY)
    prof = _product(make, fam, time_kernels=2)
    monkeypatch.delenv("SOICP_ABLATE")
    st, ms, nb = _register(prof, scan, IDENTITY)
    t = prof.timing()
    prof.close()
    return ms, nb, t


@pytest.mark.parametrize("pack", ["1", "0"])
def test_sweep(oracle, soicp, gpu_slam_factory, monkeypatch, pack):
    """production and instrumented instantiation, packed light chunks on / off: every list and status byte, and the second passes ran"""
    fam, exp, om, scan, ref, corrs = _setup(oracle, gpu_slam_factory)
    assert _state["n_checked"] == len(spd.BOUNDED_KINDS) * len(spd.CHUNK_CLASSES)
    monkeypatch.setenv("SOICP_KNN_PACK", pack)
    rf, ridx, rd2, rnbr, _ = ref
    want = _expect_status(fam, (rf, ridx, rd2, rnbr))
    slam = _product(gpu_slam_factory, fam)
    st, ms, nb = _register(slam, scan, IDENTITY)
    slam.close()
    assert not (st.flags & soicp.FLAG_QUERY_WAVES)
    ms_p, nb_p, t = _prof(gpu_slam_factory, monkeypatch, fam, scan)
    for who, m, n in (("production", ms, nb), ("instrumented", ms_p, nb_p)):
        assert np.array_equal(m, corrs["status"]), (pack, who, "status bytes against the oracle")
        assert np.array_equal(m == 1, want == 1) and np.array_equal(m == 2, want == 2), (pack, who)
        k = _check_lists(exp, scan, m, n, want == 0, rnbr, ridx, (pack, who, "numpy"))
        _check_lists(exp, scan, m, n, want == 0, corrs["nbr"].reshape(-1, 5, 3), None, (pack, who, "oracle"))
        assert k > 500
    for s in fam.info["sites"]:  # by name: TOO_FAR on exactly the e sites' special queries
        sp = slice(s["first_query"], s["first_query"] + s["n_special"])
        assert ((ms[sp] == 2).all() if s["kind"].startswith("e_") else np.isin(ms[sp], JUDGED).all()), (pack, s["name"], ms[sp])
    sites = fam.info["sites"]
    filler_chunks = -(-(len(scan) - len(fam.queries)) // 64)
    n_chunks = len(sites) + filler_chunks
    n_light = sum(s["cls"] == "light" for s in sites)
    print(f"pack={pack}: group passes {t.knn_group_passes} (chunks {n_chunks}), fallback lanes {t.knn_fallback_lanes}, packed rows {t.knn_packed_rows} "
          f"(light chunks {n_light}), kept {t.knn_packed_kept}")
    # every ordinary / split site chunk runs a near and a full group pass (a filler chunk has no cube and runs none)
    assert t.knn_group_passes > n_chunks - filler_chunks, ("the second passes ran", t.knn_group_passes, n_chunks)
    if pack == "1":
        # knn_packed_rows counts rows with work PER PASS: every light site has work in the near and in the full pass
        assert t.knn_packed_rows >= 2 * n_light, ("packed rows with work in two passes", t.knn_packed_rows, n_light)
    limit = FALLBACK_LANES_UNBOUNDED[pack]
    assert limit is not None and t.knn_fallback_lanes <= limit, ("lanes left to the exact scan", t.knn_fallback_lanes, "with SO_KNN_BOUNDED_FULL=0:", limit)


def test_sequence_entry(oracle, soicp, gpu_slam_factory):
    """the same scan twice through so_icp_register_sequence: frame 1 starts with the chained BEGIN launch, from the guess the device formed;
    its status bytes and lists equal the oracle's at that guess"""
    fam, exp, om, scan, ref, corrs = _setup(oracle, gpu_slam_factory)
    slam = _product(gpu_slam_factory, fam)
    deltas = np.tile(IDENTITY, (2, 1))
    rc, poses, guesses, stats, n_done = slam.register_sequence([scan, scan], IDENTITY, deltas)
    assert rc == 0 and n_done == 2, slam.last_error()
    ms, nb = slam.match_status(len(scan)), slam.neighbours(len(scan))
    slam.close()
    assert stats[1].flags & soicp.FLAG_CHAINED, hex(stats[1].flags)
    assert not (stats[1].flags & soicp.FLAG_QUERY_WAVES)
    orc, _, _, c1 = om.register(scan, guesses[1], oracle.default_config(max_iterations=1), want_corrs=True)
    assert orc == 0
    assert np.array_equal(ms, c1["status"]), "status bytes against the oracle at the chained guess"
    j = np.isin(ms, JUDGED)
    want = c1["nbr"].reshape(-1, 5, 3)
    got = exp[_export_index(exp, nb[j].astype(np.int64), ked.cube_of(want[j][:, 0]))]
    assert np.array_equal(got.view(np.uint32), want[j].view(np.uint32)), "neighbour lists against the oracle at the chained guess"
    assert j.sum() > 100


# knn_fallback_lanes of the instrumented, binned-ahead registration of test_pending_lanes_of_one_chunk_in_two_cubes on the
# -DSO_KNN_BOUNDED_FULL=0 library, per SOICP_KNN_PACK (same README section)
FALLBACK_LANES_UNBOUNDED_TWO_CUBES = {"1": 0, "0": 0}
N_PER_CUBE = 2100


@pytest.mark.parametrize("pack", ["1", "0"])
def test_pending_lanes_of_one_chunk_in_two_cubes(oracle, soicp, gpu_slam_factory, monkeypatch, pack):
    """(h) A scan of 2 x 2100 points and nothing else: the special queries of the `a` sites (cube (0, 0, 0)) and of the `f` sites (cube
    (1, 0, 0)), taken in turns and repeated.  Announced and binned ahead under a pose 100 m away (knn_edge_data.xruns' recipe) every
    point lands in the one 'no cube' bucket, which is cut into 65 chunks of 64 and one of 40 in the arrival order of the binning.
    Whatever that order is, some chunk holds lanes of BOTH cubes: chunks of one cube only would need 2100 = 64 k or 64 k + 40, and
    2100 = 64 * 32 + 52.  (In practice nearly every chunk is mixed.)  Every lane is pending after the near pass, so the full pass of a
    mixed chunk runs one group per cube, every lane with its own radius.
    Production and instrumented instantiation, each repeated until its scan WAS binned ahead (the host's timing decides); every
    repetition is compared bit for bit with the brute force and the oracle.  On the instrumented, binned-ahead registration the
    counters must show the second passes -- 66 chunks with a near and a full pass each, and two more for one mixed chunk -- and no
    more lanes left to the exact scan than without the bound.
    Only queries whose 5th and 6th neighbour are far apart are used: a chunk that is not compact can span metres, where the block-local
    fp32 keys are coarser than the certificate assumes (profiles/knn_second_pass/README.md, section 5)."""
    fam, exp, om, scan, ref, corrs = _setup(oracle, gpu_slam_factory)
    monkeypatch.setenv("SOICP_KNN_PACK", pack)
    special = lambda s: fam.queries[s["first_query"]:s["first_query"] + s["n_special"]]
    qa = np.concatenate([special(s) for s in fam.info["sites"] if s["kind"] == "a"])
    qf = np.concatenate([special(s) for s in fam.info["sites"] if s["kind"] == "f"])
    assert N_PER_CUBE % 64 not in (0, (2 * N_PER_CUBE) % 64), "no way to cut the bucket into chunks of one cube each"
    B_np = np.ascontiguousarray(np.stack([qa[np.arange(N_PER_CUBE) % len(qa)], qf[np.arange(N_PER_CUBE) % len(qf)]], 1).reshape(-1, 3), np.float32)
    cubes = ked.cube_of(B_np)
    assert len(B_np) > 4096 and (cubes[0::2] == (0, 0, 0)).all() and (cubes[1::2] == (1, 0, 0)).all()
    rf, ridx, rd2, rnbr, tail = ked.brute_knn(exp, B_np, n_tail=1)
    want = _expect_status(fam, (rf, ridx, rd2, rnbr))
    assert (want == 0).all(), "every query has five neighbours inside the gate"
    assert (tail[:, 5] - tail[:, 4] > 1e-3).all(), "5th and 6th neighbour far apart"
    i_all = np.arange(len(fam.queries))
    pend = np.concatenate([i_all[s["first_query"]:s["first_query"] + s["n_special"]] for s in fam.info["sites"] if s["kind"] in ("a", "f")])
    d5_near, _ = spd.near_block_fifth(fam, exp)
    assert (np.sqrt(d5_near[pend]) > spd.R_NEAR).all(), "the near pass can finish none of them"
    orc, _, _, cb = om.register(B_np, IDENTITY, oracle.default_config(max_iterations=1), want_corrs=True)
    assert orc == 0
    n_chunks = -(-len(B_np) // 64)
    for who in ("production", "instrumented"):
        if who == "instrumented":
            monkeypatch.setenv("SOICP_ABLATE", ABLATE_STATS_ONLY)
        slam = _product(gpu_slam_factory, fam, **({"time_kernels": 2} if who == "instrumented" else {}))
        monkeypatch.delenv("SOICP_ABLATE", raising=False)
        A, B = slam.host_alloc_like(fam.info["scan_a"]), slam.host_alloc_like(B_np)
        ahead = 0
        for attempt in range(16):
            slam.stage_scan(B)
            rc, _, _ = slam.register(A, fam.info["pose_a"])
            assert rc == 0, slam.last_error()
            slam.reset_timing()
            st, ms, nb = _register(slam, B, IDENTITY)
            assert not (st.flags & soicp.FLAG_QUERY_WAVES)
            assert np.array_equal(ms, cb["status"]), (pack, who, attempt)
            _check_lists(exp, B_np, ms, nb, want == 0, rnbr, ridx, (pack, who, attempt, "numpy"))
            _check_lists(exp, B_np, ms, nb, want == 0, cb["nbr"].reshape(-1, 5, 3), None, (pack, who, attempt, "oracle"))
            if st.flags & soicp.FLAG_BINNED_AHEAD:
                ahead += 1
                if who == "instrumented":
                    t = slam.timing()
                    print(f"two cubes pack={pack}: binned ahead in round {attempt + 1}, group passes {t.knn_group_passes} (chunks {n_chunks}), "
                          f"fallback lanes {t.knn_fallback_lanes}, packed rows {t.knn_packed_rows}")
                    assert t.knn_group_passes >= 2 * n_chunks + 2, ("a near and a full pass per chunk, a group per cube in the mixed one", t.knn_group_passes)
                    limit = FALLBACK_LANES_UNBOUNDED_TWO_CUBES[pack]
                    assert limit is not None and t.knn_fallback_lanes <= limit, ("lanes left to the exact scan", t.knn_fallback_lanes,
                                                                               "with SO_KNN_BOUNDED_FULL=0:", limit)
                break
        slam.close()
        assert ahead >= 1, (pack, who, "the scan was never binned ahead: no chunk of two cubes was formed")
