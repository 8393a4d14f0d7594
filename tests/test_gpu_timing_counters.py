"""-m gpu: the counters of so_icp_get_timing under time_kernels = 1 (events on the k-NN sweeps only), through so_icp_register and
so_icp_register_sequence on one context.

so_icp_register samples every third registration (registrations % 3 == 0 at its start) and counts only the sweeps that did real work: the
sweep speculated behind the converged iteration is a no-op and is left out.  so_icp_register_sequence times the first registration of a call
(k % 7 == 0) and counts its sweeps of iterations below n_iterations.  Nothing else is bracketed in mode 1: eval and prep stay at zero.

Written against the commit before the host path was split into a plan and short functions, which satisfies every assertion below as it
stands (single calls of 2, 3, 2, 2 outer iterations: knn_launches 2, 2, 2, 4; the sequence adds 2, the iterations of its first scan)."""
import numpy as np
import pytest

from helpers import chain_deltas
from superodom_amd import synth

pytestmark = pytest.mark.gpu


def test_mode_1_counts_the_real_sweeps_of_the_sampled_registrations(soicp, gpu_slam_factory):
    sc = synth.Scene("tiny")
    slam = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=5, time_kernels=1)
    slam.add_surf_point_cloud(sc.map_points)
    ids = [0, 1, 2, 3, 4, 5]
    scans = [slam.host_alloc_like(np.ascontiguousarray(sc.scan(i), dtype=np.float32)) for i in ids]

    def single(i):
        rc, _, st = slam.register(scans[i], sc.guess(i))
        assert rc == 0 and st.n_iterations >= 1, (i, rc, slam.last_error())
        t = slam.timing()
        print("single call", i, "n_iterations", st.n_iterations, "registrations", t.registrations, "knn_launches", t.knn_launches, "knn_ms_total", t.knn_ms_total)
        return st, t

    st1, t1 = single(0)  # registrations == 0 at its start: sampled
    assert t1.registrations == 1
    assert t1.knn_launches == st1.n_iterations  # (the speculated no-op sweep is not counted)
    assert t1.knn_ms_total > 0
    _, t2 = single(1)
    _, t3 = single(2)
    assert t2.knn_launches == t1.knn_launches and t3.knn_launches == t1.knn_launches
    assert t3.registrations == 3
    st4, t4 = single(3)  # registrations == 3 at its start: sampled again
    assert t4.registrations == 4
    assert t4.knn_launches == t3.knn_launches + st4.n_iterations
    assert t4.knn_ms_total > t3.knn_ms_total

    rc, _, _, stats, n_done = slam.register_sequence(scans, sc.guess(0), chain_deltas(sc, ids))
    assert rc == 0 and n_done == len(ids), (rc, n_done, slam.last_error())
    t5 = slam.timing()
    iters = [st.n_iterations for st in stats]
    print("sequence n_iterations", iters, "flags", [hex(st.flags) for st in stats], "registrations", t5.registrations, "knn_launches", t5.knn_launches)
    assert t5.registrations == t4.registrations + len(ids)
    grew = t5.knn_launches - t4.knn_launches
    assert iters[0] <= grew <= sum(iters), (grew, iters)
    assert t5.eval_launches == 0 and t5.prep_launches == 0
    slam.close()
