"""The path-directed k-NN inputs (knn_edge_data.py) on the CPU: for every family and EVERY query the oracle's exact search -- grid
and exhaustive -- equals the plain numpy restatement in neighbour coordinates and in the bits of d2; and every family has the
property that makes it worth running on the device (printed, then asserted).  Every comparison is exact.  For the families at the
distance gate, on interior cell faces and on the coarser grids the oracle is held to the brute force for k = 1 .. 5 as well, the
sites to what they claim to be (which side of the gate, which cell, one float apart), the oracle to status 1 on non-finite scan
rows; and the model of the selection key's fp32 distance stays below kApproxAbsErr (read from kernels.hip) on all of them."""
import hashlib
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import knn_edge_data as ked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _load(oracle, fam):
    om = oracle.OracleMap(plane_res=fam.plane_res)
    om.add_surf(fam.map_points, raw=False)  # THROUGH the voxel filter, like the product's map
    return om


@pytest.mark.parametrize("name", list(ked.FAMILIES))
def test_oracle_equals_the_numpy_reference_and_the_family_has_its_property(oracle, name):
    fam = ked.family(name)
    om = _load(oracle, fam)
    exp = om.export()
    # nothing is merged or moved by the voxel filter: the loaded map is the generated one, point for point
    assert len(exp) == len(fam.map_points)
    order = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
    assert np.array_equal(order(exp).view(np.uint32), order(fam.map_points).view(np.uint32))
    assert len(np.unique(exp, axis=0)) == len(exp)
    q = fam.queries
    found, idx, d2, nbr, tail = ked.brute_knn(exp, q, n_tail=8)
    idx_all = ked.brute_knn(exp, q, k=6)[1] if name == "near_ties" else None
    for use_grid in (1, 0):
        of, onbr, od2, oidx, _ = om.knn(q, 5, use_grid=use_grid)
        assert np.array_equal(of.astype(bool), found), (name, use_grid)
        f = found
        assert np.array_equal(od2[f].view(np.uint32), d2[f].view(np.uint32)), (name, use_grid)
        assert np.array_equal(onbr[f].view(np.uint32), nbr[f].view(np.uint32)), (name, use_grid)
    if name in ked.NEW_FAMILIES or name == "faces":  # (faces: the cubes of 1, 2 and 3 points)
        for k in (1, 2, 3, 4):
            kf, kidx, kd2, knbr = ked.brute_knn(exp, q, k=k)
            for use_grid in (1, 0):
                of, onbr, od2, oidx, _ = om.knn(q, k, use_grid=use_grid)
                assert np.array_equal(of.astype(bool), kf), (name, k, use_grid)
                assert np.array_equal(od2[kf].view(np.uint32), kd2[kf].view(np.uint32)), (name, k, use_grid)
                assert np.array_equal(onbr[kf].view(np.uint32), knbr[kf].view(np.uint32)), (name, k, use_grid)
    # ---- the family's property
    full = found & (d2[:, 4] < 1e30)
    tie56 = full & (tail[:, 4] == tail[:, 5])
    n_equal_at_5 = (tail == tail[:, 4:5]).sum(1)  # candidates at exactly the 5th distance
    print(f"{name}: {len(exp)} map points, {len(q)} queries, {int(found.sum())} with a cube, {int(full.sum())} with five neighbours, "
          f"{int(tie56.sum())} with d2[4] == d2[5], {int((n_equal_at_5 >= 8).sum())} with >= 8 equal distances at rank 5")
    if name.startswith("ties"):
        assert tie56.sum() >= 0.25 * len(q), (name, tie56.sum(), len(q))
        if fam.info["power_of_two"]:
            assert (full & (n_equal_at_5 >= 8)).sum() > 0, name
    if name == "near_ties":
        near = (np.abs(tail - tail[:, 4:5]) <= 2e-5).sum(1)
        print(f"{name}: candidates within 2e-5 m^2 of the 5th distance: min {near.min()}")
        assert full.all() and (near >= 9).all()
        # ranks 5 and 6 exactly one float ulp apart wherever the site's pattern says so, and the whole pattern in ulps
        bits = tail[:, :12].astype(np.float32).view(np.uint32).astype(np.int64)
        assert np.array_equal(bits - bits[:, :1], fam.info["patterns"]), "the tuned d2 pattern of every site"
        assert ((bits[:, 5] - bits[:, 4]) == 1).sum() >= len(q) // 2
        # every site holds a pair -- its exact 5th and 6th neighbour -- that the block-local fp32 distance of the selection key puts
        # in the reverse order; and the two are never more than the key's error bound apart, so no key can be trusted with them
        rev = 0
        for i in range(len(q)):
            a = ked.approx_d2_block_local(q[i], exp[idx_all[i, 4:6]], fam.plane_res)
            assert tail[i, 4] < tail[i, 5] and a[0] > a[1], (i, a, tail[i, 4:6])
            rev += int((a[0].view(np.uint32) & ked.KEY_KEEP) > (a[1].view(np.uint32) & ked.KEY_KEEP))
        print(f"{name}: approximate order of the exact 5th / 6th neighbour reversed at all {len(q)} sites, at {rev} of them in the key's kept bits too")
    if name == "xruns":
        nc, cell = ked.grid_cells(fam.plane_res)
        n1 = fam.info["n_one"]
        cells = np.floor((q.astype(np.float64) + 25.0) % 50.0 / cell).astype(np.int64)
        assert len(np.unique(ked.cube_of(q[:n1]), axis=0)) == 1 and len(np.unique(ked.cube_of(q[n1:]), axis=0)) == 8
        span = cells[:n1].max(0) - cells[:n1].min(0) + 1
        print(f"{name}: one-cube queries span {span} cells; any 9 of them span, at the 1st percentile, "
              f"{np.percentile([np.prod(np.ptp(cells[:n1][np.random.default_rng(k).choice(n1, 9, replace=False)][:, 1:], axis=0) + 2) for k in range(300)], 1):.0f} x-runs")
        assert span[1] * span[2] > 32 and n1 % 64 == 9
        wa = fam.info["scan_a"].astype(np.float64) + fam.info["pose_a"][:3]
        assert len(np.unique(ked.cube_of(wa), axis=0)) == 1 and ked.cell_counts(exp, wa.astype(np.float32)).min() > 50
        assert len(np.unique(np.floor((wa + 25.0) % 50.0 / (cell / 2)).astype(np.int64), axis=0)) > 4096, "one light chunk per point of scan A"
        assert ked.cell_counts(exp, (q.astype(np.float64) + fam.info["pose_a"][:3]).astype(np.float32)).max() == 0, "under pose A scan B meets no cube"
    if name == "dense":
        # the candidates of every site's block, counted the way the device grid files them (fp64 cell of the point's own coordinates)
        nc, cell = ked.grid_cells(fam.plane_res)
        assert nc == 64
        at = 0
        seen = set()
        for cu, h, kcount, nq in fam.info["sites"]:
            mn = np.array(cu, float) * 50.0 - 25.0
            c = np.floor((exp.astype(np.float64) - mn) * (nc / 50.0)).astype(np.int64)
            in_block = ((c >= np.array(h)) & (c <= np.array(h) + 1)).all(1) & (ked.cube_of(exp) == np.array(cu)).all(1)
            assert in_block.sum() == kcount, (cu, h, kcount, int(in_block.sum()))
            qs = q[at:at + nq]; at += nq
            u = (qs.astype(np.float64) - mn) / cell
            assert (np.floor(u) == np.array(h)).all() and (u - np.floor(u) >= 0.5).all(), "queries in the upper octant of the home cell"
            seen.add((kcount, nq))
        assert at == len(q) and seen == set(ked.DENSE_SITES)
        assert full.all()
    if name.startswith("faces"):
        nf = fam.info["n_face_queries"]
        across = ked.nearest_across(exp, q[:nf])
        print(f"{name}: {nf} queries at faces, edges and corners; nearest point across the face at d2 <= {across.max():.4f}, "
              f"in-cube 5th neighbour at d2 >= {d2[:nf, 4].min():.4f}")
        assert found[:nf].all() and (across < d2[:nf, 4]).all(), "a map point across the face is strictly nearer than the in-cube 5th neighbour"
        counts = ked.cell_counts(exp, q)
        assert {1, 2, 3, 4, 5, 6} <= set(counts.tolist()) and (~found).sum() >= 4
        assert (np.abs(q[:nf].astype(np.float64)) % 50.0 - 25.0 == 0).any(), "queries exactly on a face"


def test_the_reference_is_independent_and_deterministic():
    a, b = ked.FAMILIES["faces"](), ked.FAMILIES["faces"]()
    assert np.array_equal(a.map_points, b.map_points) and np.array_equal(a.queries, b.queries)
    # three points, one query: hand-checked order with an exact tie (indices 0 and 2 at the same distance)
    mp = np.array([[1, 0, 0], [0, 0.5, 0], [-1, 0, 0]], np.float32)
    found, idx, d2, nbr = ked.brute_knn(mp, np.zeros((1, 3), np.float32))
    assert found[0] and idx[0].tolist() == [1, 0, 2, 0, 0] and d2[0, 4] == ked.FLT_MAX and d2[0, :3].tolist() == [0.25, 1.0, 1.0]


# ------------------------------------------------------------------------------------------------------------------------
# the families at the distance gate, on the cell faces of every grid, and the non-finite rows
# ------------------------------------------------------------------------------------------------------------------------
def test_faces_at_0_2_is_the_family_it_was():
    """what the family held before it took planeRes as a parameter (hashes taken from that version), byte for byte; behind it only the
    cubes of 1, 2 and 3 points"""
    fam = ked.family("faces")
    n, m = fam.info["n_map_v1"], fam.info["n_queries_v1"]
    assert (n, m) == (64167, 3542) and (len(fam.map_points), len(fam.queries)) == (n + 6, m + 12)
    assert hashlib.sha256(fam.map_points[:n].tobytes()).hexdigest() == "daaf8f046d3ac1b046d95f527320cbc6a8e4ed78d3b75cd3844ad8203e231e4a"
    assert hashlib.sha256(fam.queries[:m].tobytes()).hexdigest() == "b8c75bc89d7594ff5203f4587f6189ad0d287926bfb9ff3384d4a7c587ff5e6d"
    assert sorted(np.unique(ked.cube_of(fam.map_points[n:])[:, 0], return_counts=True)[1].tolist()) == [1, 2, 3]


@pytest.mark.parametrize("plane_res", ked.GATE_RES)
def test_gate_sites_are_what_they_claim(plane_res):
    """26 directions x 4 placements x 2 sides, none dropped; the brute force puts the fifth neighbour of every `in` site on or inside
    the gate and that of every `out` site outside; a pair is one configuration, moved by a whole number of cells, that differs in ONE
    coordinate of the fifth point by ONE float; the fifth lies beyond half a cell (no near pass can certify it), and in the cell the
    placement names"""
    fam = ked.family(f"gate_edge_{plane_res}")
    sites, gate, q, mp = fam.info["sites"], fam.info["gate"], fam.queries, fam.map_points
    nc, cell = ked.grid_cells(plane_res)
    assert gate == np.float32(3) * np.float32(plane_res) and gate.dtype == np.float32
    names = [s["name"] for s in sites]
    want = [f"{''.join('-0+'[v + 1] for v in d)}/{pl}/{side}" for d in ked.GATE_DIRECTIONS for pl in ked.GATE_PLACEMENTS for side in ("in", "out")]
    assert names == want and len(set(names)) == 208 and len(ked.GATE_DIRECTIONS) == 26
    assert [s["query"] for s in sites] == list(range(208)) and len(q) == 208
    found, idx, d2, nbr, tail = ked.brute_knn(mp, q, n_tail=1)
    assert found.all()
    n_equal = 0
    for s_in, s_out in zip(sites[0::2], sites[1::2]):
        assert (s_in["side"], s_out["side"]) == ("in", "out") and s_in["name"][:-3] == s_out["name"][:-4]
        a, b = s_in["query"], s_out["query"]
        # -- as built
        assert idx[a, 4] == s_in["fifth"] and d2[a, 4] <= gate and tail[a, 5] > gate * 1.5, s_in["name"]
        assert d2[a, 3] < 0.75 * gate and d2[b, 3] < 0.75 * gate, "four clearly nearer"
        assert idx[b, 4] == s_out["fifth"] and d2[b, 4] > gate, s_out["name"]
        assert np.nextafter(d2[a, 4], np.float32(np.inf)) > gate or d2[a, 4] == gate
        assert s_in["equal"] == bool(d2[a, 4] == gate)
        n_equal += s_in["equal"]
        assert s_out["sixth"] == (tail[b, 5] < 2.0 * gate) and not s_in["sixth"], "every other out site has a sixth point, at 1.3 r"
        if s_out["sixth"]:
            assert tail[b, 5] > 1.5 * gate
        # -- one float apart: the out site minus the shift IS the in site, but for one step of the fifth's tuned coordinate
        sh = np.zeros(3); sh[s_in["shift_axis"]] = fam.info["shift"]
        assert abs(fam.info["shift"] / cell - round(fam.info["shift"] / cell)) < 1e-12, "a whole number of cells"
        back = lambda p: (p.astype(np.float64) - sh).astype(np.float32)
        assert np.array_equal(back(q[b]).astype(np.float64) + sh, q[b].astype(np.float64)) and np.array_equal(back(q[b]), q[a])
        pa, pb = mp[s_in["first_point"]:s_in["first_point"] + 5], mp[s_out["first_point"]:s_out["first_point"] + 5]
        assert np.array_equal(back(pb).astype(np.float64) + sh, pb.astype(np.float64)), "the shift is exact in float"
        diff = np.argwhere(back(pb) != pa)
        t = s_in["tuned_axis"]
        assert diff.tolist() == [[4, t]], (s_in["name"], diff)
        away = np.float32(np.inf) * np.sign(pa[4, t] - q[a, t])
        assert np.nextafter(pa[4, t], away) == back(pb)[4, t], "the adjacent float, away from the query"
        # -- where it lies
        for s, qi in ((s_in, a), (s_out, b)):
            p5 = mp[s["fifth"]]
            assert np.sqrt(d2[qi, 4]) > 0.5 * cell * 1.2
            assert (ked.cube_of(mp[s["first_point"]:s["first_point"] + s["n_points"]]) == ked.cube_of(q[qi])).all()
            d = np.array(s["direction"])
            cq, c5 = ked.cell_of(q[qi], plane_res), ked.cell_of(p5, plane_res)
            u = (q[qi].astype(np.float64) + 25.0) % 50.0 / cell - cq  # position inside the cell, 0 .. 1
            if s["placement"] == "cell_middle":
                assert (np.abs(u - 0.5) < 1e-3 / cell).all()
            if s["placement"] == "cell_face":
                assert c5[t] == cq[t] + d[t] and min(u[t], 1 - u[t]) * cell <= 1e-3
                w = (p5[t].astype(np.float64) + 25.0) % 50.0 / cell - c5[t]
                assert (w if d[t] > 0 else 1 - w) > (0.9 if np.abs(d).sum() == 1 else 0.5), "in the far part of the next cell (along an axis: its last tenth)"
            if s["placement"] == "cell_corner":
                assert np.array_equal(c5, cq + d) and (np.minimum(u, 1 - u) * cell <= 1e-3).all()
            if s["placement"] == "cube_face":
                f = (t + 2) % 3
                assert np.abs(np.abs(q[qi, f].astype(np.float64) - (100.0 if t == 1 else -100.0 if t == 2 else 0.0)) - 25.0) <= 1e-3
    print(f"gate_edge {plane_res}: {nc} cells of {cell:.6f} m, gate {gate!r}, {n_equal} of 104 in-sites with d2[4] == gate exactly")
    assert n_equal == fam.info["n_equal"] and n_equal >= 26
    dist = np.sqrt(((q[:, None, :].astype(np.float64) - q[None, :, :]) ** 2).sum(2)) + 1e9 * np.eye(len(q))
    assert dist.min() >= 4.0
    filler = np.array([3.0, 40.0, 9.0]) + np.arange(4200 - 208)[:, None] * np.array([0.001, 0, 0])
    clear = np.sqrt(((mp[:, None, :].astype(np.float64) - filler[None, ::50, :]) ** 2).sum(2)).min()
    assert clear > 2 * np.sqrt(3 * 0.8), clear
    # the far registration of the binned-ahead test (as xruns)
    wa = fam.info["scan_a"].astype(np.float64) + fam.info["pose_a"][:3]
    assert len(np.unique(ked.cube_of(wa), axis=0)) == 1 and ked.cell_counts(mp, wa.astype(np.float32)).min() > 50
    assert len(np.unique(np.floor((wa + 25.0) % 50.0 / (cell / 2)).astype(np.int64), axis=0)) > 4096, "one light chunk per point of scan A"
    assert ked.cell_counts(mp, (q.astype(np.float64) + fam.info["pose_a"][:3]).astype(np.float32)).max() == 0, "under pose A scan B meets no cube"


@pytest.mark.parametrize("plane_res", ked.CELL_FACE_RES)
def test_cell_face_points_lie_in_the_cells_the_family_names(plane_res):
    """the fp64 cell of every point (info) is its cell in exact rational arithmetic; on every face, on every axis, a float-adjacent
    pair of map points and one of queries lie in different cells; every list reaches across a cell face"""
    fam = ked.family(f"cell_faces_{plane_res}")
    nc, cell = ked.grid_cells(plane_res)
    assert nc == {0.25: 57, 0.4: 45}[plane_res]
    on_upper_face = 0
    for pts, cells in ((fam.map_points, fam.info["map_cells"]), (fam.queries, fam.info["query_cells"])):
        assert (ked.cube_of(pts) == 0).all()
        for p, c in zip(pts.tolist(), cells.tolist()):
            for a in range(3):
                lo = Fraction(-25) + c[a] * Fraction(50, nc)
                # (a coordinate EXACTLY on a face -- 5.0 on the 45-cell grid -- may be filed below it: the product's grid is the fp64
                #  expression, (x - min) * (1 / cell), for map points and queries alike, and 30 * (1 / (50 / 45)) is 26.999...)
                assert lo <= Fraction(p[a]) <= lo + Fraction(50, nc), (p, c)
                on_upper_face += Fraction(p[a]) == lo + Fraction(50, nc)
    for k, (exact, below, at) in fam.info["face_values"].items():
        assert np.nextafter(below, np.float32(np.inf)) == at and Fraction(float(below)) < exact <= Fraction(float(at))
        for a in range(3):
            for pts, cells in ((fam.map_points[:fam.info["n_on_faces"]], fam.info["map_cells"]), (fam.queries, fam.info["query_cells"])):
                lo, hi = cells[:len(pts)][pts[:, a] == below, a], cells[:len(pts)][pts[:, a] == at, a]
                assert len(lo) and len(hi) and (lo == k - 1).all() and (hi == k).all(), (plane_res, k, a)
    found, idx, d2, nbr = ked.brute_knn(fam.map_points, fam.queries)
    across = (fam.info["map_cells"][idx] != fam.info["query_cells"][:, None, :]).any(2)
    on_face = idx < fam.info["n_on_faces"]
    print(f"cell_faces {plane_res}: {nc} cells, {len(fam.queries)} queries, neighbours in another cell per list {across.sum(1).mean():.2f}, "
          f"lists with a neighbour ON a face {on_face.any(1).mean():.2f}; coordinates exactly on a face and filed below it: {on_upper_face}")
    assert found.all() and (d2[:, 4] < ked.gate_of(plane_res)).all() and across.any(1).all() and on_face.any(1).mean() > 0.5


def test_oracle_gives_nonfinite_rows_status_1_and_leaves_the_rest(oracle):
    fam = ked.family("faces")
    om = _load(oracle, fam)
    scan = fam.queries
    bad, rows = ked.nonfinite_rows(scan)
    assert len(rows) == 84 and rows[0] == 0 and rows[-1] == len(scan) - 1 and {63, 64} <= set(rows.tolist())
    runs = np.split(rows, np.nonzero(np.diff(rows) > 1)[0] + 1)
    assert sorted(map(len, runs)) == [1, 1, 2, 16, 64]
    changed = (bad.view(np.uint32) != scan.view(np.uint32))
    assert np.array_equal(np.nonzero(changed.any(1))[0], rows) and (changed.sum(1) <= 1).all()
    vals = bad[changed]
    assert np.isnan(vals).sum() == 21 and (vals == np.inf).sum() == 21 and (vals == -np.inf).sum() == 21 and (vals == np.float32(1e12)).sum() == 21
    for a in range(3):
        assert {"nan", "inf", "-inf", "1e12"} == {"nan" if np.isnan(v) else "1e12" if v == np.float32(1e12) else str(float(v)) for v in bad[changed[:, a], a]}
    cfg1 = oracle.default_config(max_iterations=1)
    rc0, _, _, clean = om.register(scan, IDENTITY, cfg1, want_corrs=True)
    rc1, _, _, dirty = om.register(bad, IDENTITY, cfg1, want_corrs=True)
    assert rc0 == 0 and rc1 == 0
    assert (dirty["status"][rows] == 1).all()
    rest = np.setdiff1d(np.arange(len(scan)), rows)
    assert np.array_equal(dirty["status"][rest], clean["status"][rest]) and np.array_equal(dirty["nbr"][rest].view(np.uint32), clean["nbr"][rest].view(np.uint32))
    assert (clean["status"][rows] != 1).sum() > 60, "rows that had a cube and a status of their own"


def kernel_constant(name):
    src = open(os.path.join(ROOT, "superodom_amd", "csrc", "kernels.hip")).read()
    return float(re.search(rf"constexpr float {name} = ([0-9.eE+-]+)f;", src).group(1))


@pytest.mark.parametrize("name", ked.NEW_FAMILIES)
def test_the_selection_keys_distance_stays_inside_its_error_bound(name):
    """the model of the selection key's fp32 block-local distance (approx_d2_block_local) against the exact d2 of the float
    coordinates, over every candidate within 1.15 r of every query of the family: the worst difference, printed per grid (DESIGN
    section 6 quotes it), stays below the bound the certificate subtracts (kApproxAbsErr, kernels.hip).  Shown on these inputs, not
    proven for all."""
    fam = ked.family(name)
    bound = kernel_constant("kApproxAbsErr")
    assert 0 < bound < 1e-4
    mp, q = fam.map_points, fam.queries
    reach2 = (1.15 ** 2) * float(ked.gate_of(fam.plane_res))
    mc, qc = ked.cube_of(mp), ked.cube_of(q)
    worst, n_cand, where = 0.0, 0, None
    cubes, minv = np.unique(mc, axis=0, return_inverse=True)
    minv = minv.reshape(-1)
    members = {tuple(c): mp[minv == i] for i, c in enumerate(cubes)}
    for i in range(len(q)):
        cand = members.get(tuple(qc[i]))
        if cand is None:
            continue
        d = cand.astype(np.float64) - q[i].astype(np.float64)
        exact = (d * d).sum(1)
        near = exact <= reach2
        if not near.any():
            continue
        err = np.abs(ked.approx_d2_block_local(q[i], cand[near], fam.plane_res).astype(np.float64) - exact[near])
        n_cand += int(near.sum())
        if err.max() > worst:
            worst, where = float(err.max()), q[i]
    nc, cell = ked.grid_cells(fam.plane_res)
    print(f"{name}: planeRes {fam.plane_res}, {nc} cells of {cell:.4f} m: worst |approximate - exact| d2 {worst:.2e} over {n_cand} candidates "
          f"(at query {where}); bound {bound:.1e}")
    assert n_cand > 1000 and worst < bound, (name, worst, bound)
