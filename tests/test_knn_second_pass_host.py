"""The sites of knn_second_pass_data.bounded() are what their names say (no GPU): every precondition the device test relies on, judged
by the numpy brute force on the map in an emulated canonical order."""
import numpy as np

import knn_edge_data as ked
import knn_second_pass_data as spd


def test_bounded_sites_hold_their_preconditions():
    fam = spd.bounded()
    exp = spd.canonical_order(fam.map_points)
    ref = ked.brute_knn(exp, fam.queries, n_tail=2)
    assert spd.check_sites(fam, exp, ref) == len(spd.BOUNDED_KINDS) * len(spd.CHUNK_CLASSES)
    # far from the filler line of the device tests' scans (y = 40, z = 9) and from the patch of the binned-ahead recipe
    assert (np.abs(fam.map_points[:fam.info["n_site_points"], 1]) < 26).all()


def test_radius_of_the_bounded_pass():
    """r_lane in the kernel's float arithmetic: the gate radius without a fifth and beyond the gate, sqrt(d5) * 1.0005 + 1e-4 below it"""
    g = float(spd.r_gate())
    assert abs(g - (np.sqrt(0.6) * 1.0005 + 1e-4)) < 1e-6
    r = spd.r_lane([np.inf, 0.64, 0.45 ** 2, 0.0])
    assert r[0] == r[1] == spd.r_gate() and abs(float(r[2]) - (0.45 * 1.0005 + 1e-4)) < 1e-6 and abs(float(r[3]) - 1e-4) < 1e-9
    assert (r.astype(np.float64) ** 2 > np.array([np.inf, 0.64, 0.45 ** 2, 0.0]) * (1 + 1e-5))[2:].all(), "the certificate's cover r_lane^2 (1 - 1e-6) stays above d5"
