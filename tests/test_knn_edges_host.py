"""The path-directed k-NN inputs (knn_edge_data.py) on the CPU: for every family and EVERY query the oracle's exact search -- grid
and exhaustive -- equals the plain numpy restatement in neighbour coordinates and in the bits of d2; and every family has the
property that makes it worth running on the device (printed, then asserted).  Every comparison is exact."""
import numpy as np
import pytest

import knn_edge_data as ked


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
    if name == "faces":
        nf = fam.info["n_face_queries"]
        across = ked.nearest_across(exp, q[:nf])
        print(f"{name}: {nf} queries at faces, edges and corners; nearest point across the face at d2 <= {across.max():.4f}, "
              f"in-cube 5th neighbour at d2 >= {d2[:nf, 4].min():.4f}")
        assert found[:nf].all() and (across < d2[:nf, 4]).all(), "a map point across the face is strictly nearer than the in-cube 5th neighbour"
        counts = ked.cell_counts(exp, q)
        assert {4, 5, 6} <= set(counts.tolist()) and (~found).sum() >= 4
        assert (np.abs(q[:nf].astype(np.float64)) % 50.0 - 25.0 == 0).any(), "queries exactly on a face"


def test_the_reference_is_independent_and_deterministic():
    a, b = ked.FAMILIES["faces"](), ked.FAMILIES["faces"]()
    assert np.array_equal(a.map_points, b.map_points) and np.array_equal(a.queries, b.queries)
    # three points, one query: hand-checked order with an exact tie (indices 0 and 2 at the same distance)
    mp = np.array([[1, 0, 0], [0, 0.5, 0], [-1, 0, 0]], np.float32)
    found, idx, d2, nbr = ked.brute_knn(mp, np.zeros((1, 3), np.float32))
    assert found[0] and idx[0].tolist() == [1, 0, 2, 0, 0] and d2[0, 4] == ked.FLT_MAX and d2[0, :3].tolist() == [0.25, 1.0, 1.0]
