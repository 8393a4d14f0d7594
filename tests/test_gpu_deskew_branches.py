"""-m gpu: so_icp_deskew_scan(_dev) on the path-directed cases of tests/deskew_data.py (branch_case: every branch of matrix_to_quat,
interpolated_pose and quat_slerp, tables of 511 / 512 / 513 poses either side of the LDS / global switch, clamped counts at wavefront
and workgroup edges) against the host build of the same header (tests/deskew_host.py), which tests/test_deskew_branches_host.py
holds to the C oracle bit for bit and whose census assertions say that each case reaches its branch.

The criterion is test_gpu_deskew.py's: host and device run the same fp64 operation sequence and only acos / sin inside slerp may
differ in the last bit, so more than 0.999 of the float32 values are bit-identical, none is more than one float32 spacing off, and
every point is within 1e-5 m of scipy.  A point that meets no acos / sin -- before the first entry, exactly on one, clamped, or
between neighbours on the lerp side -- gets no allowance: every bit."""
import ctypes as C

import numpy as np
import pytest

import deskew_data as dd
import deskew_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    """name -> the host build's (records, start frame, clamped count), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = deskew_host.deskew(*dd.branch_case(name).args)
        return cache[name]
    return get


def _check(c, got, info, want_all):
    want, wstart, wclamped = want_all
    q = c.census
    finite = q["finite"]
    assert info.n_clamped == wclamped == int((finite & (q["path"] == dd.CLAMPED)).sum())
    assert list(info.t_w_original_l) + list(info.q_w_original_l) == list(wstart), "the sweep-start frame is host arithmetic on both sides"
    assert np.array_equal(got[:, 12:], c.rec[:, 12:]), "only x y z are rewritten"
    assert np.array_equal(got[~finite], c.rec[~finite]), "non-finite points are left alone"
    frac, worst = dd.close_in_ulps(dd.xyz_of(got), dd.xyz_of(want))
    no_trig = finite & ((q["path"] != dd.INTERIOR) | q["lerp"] | q["exact"])
    differ = (got[:, :12] != want[:, :12]).any(1)
    print(f"{c.name}: {frac:.6f} of the values identical, worst {worst:.2f} spacings; {int(differ.sum())} of {len(got)} points differ, "
          f"{int((differ & no_trig).sum())} of {int(no_trig.sum())} points without acos / sin")
    assert frac > 0.999 and worst <= 1.0, (frac, worst)
    assert not (differ & no_trig).any(), "no acos / sin on this point's way: every bit"
    if finite.any():
        ref = dd.scipy_deskew(*c.args)
        assert np.abs(dd.xyz_of(got)[finite].astype(np.float64) - ref[finite]).max() < 1e-5


@pytest.mark.parametrize("name", dd.BRANCH_CASES)
def test_kernel_gives_the_host_builds_bits(gpu_slam_factory, host, name):
    slam = gpu_slam_factory()
    c = dd.branch_case(name)
    got, info = slam.deskew_scan(*c.args)
    _check(c, got, info, host(name))


def test_counts_do_not_carry_over_between_calls(gpu_slam_factory, host):
    """one context, sweeps of every size in turn: each call reports its own clamped count"""
    slam = gpu_slam_factory()
    for name in [f"clamp{n}" for n in dd.CLAMP_SIZES] + ["gone63", "clamp1", "gone1", "clamp65"]:
        got, info = slam.deskew_scan(*dd.branch_case(name).args)
        assert info.n_clamped == host(name)[2] and np.array_equal(got, host(name)[0]), name


@pytest.mark.parametrize("name", ["tail513"])
def test_records_resident_in_hbm(gpu_slam_factory, host, name):
    """so_icp_deskew_scan_dev on a 513-pose table that ends mid-sweep: the global-memory path, interior and clamped points"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    slam = gpu_slam_factory()
    c = dd.branch_case(name)
    rec = c.rec
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), rec.nbytes) == 0
    try:
        assert hip.hipMemcpy(d, rec.ctypes.data_as(C.c_void_p), rec.nbytes, 1) == 0  # hipMemcpyHostToDevice
        info = slam.deskew_scan_dev(d.value, rec.shape[0], rec.shape[1], c.time_off, c.t0, c.poses, c.imu, c.T_i_l)
        got = np.empty_like(rec)
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d, rec.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    finally:
        hip.hipFree(d)
    _check(c, got, info, host(name))
    staged, sinfo = slam.deskew_scan(*c.args)
    assert np.array_equal(got, staged) and info.n_clamped == sinfo.n_clamped, "the two entry points run the same kernel"
