"""-m gpu: so_icp_registered_scan(_dev) -- laserMapping::publishTopic's registered scan from resident records, transformed and
compacted in one launch -- against the restatement (tests/registered_scan_ref.py), bit for bit: the count, the kept records in
order, the context's device copy, and the input left as it was.  tests/test_registered_scan_host.py checks that the inputs used
here carry near-sensor points, drops at the world origin, non-finite coordinates and an all-dropped tile."""
import ctypes as C

import numpy as np
import pytest

import deskew_data as dd
import feature_extraction_ref as fr
import livox_ref as lr
import registered_scan_ref as rr
from superodom_amd import synth

pytestmark = pytest.mark.gpu
T0 = 1.7e9 + 0.25


class _Hip:
    def __init__(self):
        self.h = C.CDLL("libamdhip64.so")
        self.h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.h.hipFree.argtypes = [C.c_void_p]

    def upload(self, a, at=0):
        """a into a fresh allocation of at + a.nbytes bytes, `at` bytes in; returns (allocation, address of a[0])"""
        d = C.c_void_p()
        assert self.h.hipMalloc(C.byref(d), max(at + a.nbytes, 1)) == 0
        if a.nbytes:
            assert self.h.hipMemcpy(C.c_void_p(d.value + at), a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        return d, d.value + at

    def download(self, d, nbytes):
        out = np.empty(nbytes, np.uint8)
        if nbytes:
            assert self.h.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(d), nbytes, 2) == 0
        return out

    def free(self, d):
        self.h.hipFree(d)


@pytest.fixture(scope="module")
def hip():
    return _Hip()


@pytest.fixture(scope="module")
def slam(gpu_slam_factory):
    s = gpu_slam_factory(plane_res=0.2)
    yield s
    s.close()


def _dev(hip, slam, rec, T, at=0):
    """registered_scan_dev on an upload of rec `at` bytes into an allocation: (host out, downloaded *d_out, n_kept, input afterwards)"""
    n, stride = rec.shape
    d, addr = hip.upload(rec, at)
    try:
        out, d_out, nk = slam.registered_scan_dev(addr, n, stride, T)
        dev_out = hip.download(d_out, nk * stride).reshape(nk, stride) if nk else np.zeros((0, stride), np.uint8)
        after = hip.download(addr, rec.nbytes).reshape(n, stride)
    finally:
        hip.free(d)
    return out, dev_out, nk, after


def _same(got, want, what):
    if got.shape == want.shape and np.array_equal(got, want):
        return True
    print(what, "shapes", got.shape, want.shape)
    if got.shape == want.shape:
        rows = np.nonzero((got != want).any(1))[0]
        print(f"{len(rows)} of {len(got)} records differ; first: {rows[:5].tolist()}")
        for r in rows[:5]:
            print(r, got[r].view(np.uint32).tolist(), want[r].view(np.uint32).tolist())
    return False


@pytest.mark.parametrize("n", rr.SIZES)
@pytest.mark.parametrize("name", rr.FAMILIES)
def test_equals_the_restatement_bit_for_bit(hip, slam, name, n):
    rec, T, want, _, keep = rr.family(name, n)
    out, dev_out, nk, after = _dev(hip, slam, rec, T)
    assert nk == len(want) == keep.sum()
    assert _same(out, want, f"{name} {n} out"), "the first n_kept records of out"
    assert _same(dev_out, want, f"{name} {n} *d_out"), "the context's device copy"
    assert np.array_equal(after, rec), "the input records are not modified"


@pytest.mark.parametrize("name", rr.FAMILIES)
def test_equals_transform_cloud_and_a_squeeze(slam, hip, name):
    """what the node published before: so_icp_transform_cloud in place, then the kept records moved up"""
    rec, T, want, _, _ = rr.family(name, 3 * rr.TILE)
    moved, flags, nk_old = slam.transform_cloud(rec, T)
    squeezed = moved[flags.astype(bool)]
    out, dev_out, nk, _ = _dev(hip, slam, rec, T)
    assert nk == nk_old == len(squeezed) and _same(out, squeezed, name) and _same(dev_out, squeezed, name)
    assert _same(slam.registered_scan(rec, T), squeezed, name + " host entry")


@pytest.mark.parametrize("name", ["scan", "nonfinite", "tiles_middle"])
@pytest.mark.parametrize("stride", [32, 16, 12, 20, 48])
def test_strides(slam, hip, name, stride):
    """32, 16 and 48 from an aligned base take the 16-byte instantiation, 12 and 20 the dword one"""
    for n in (257, 2 * rr.TILE + 77):
        rec, T, want, _, _ = rr.family(name, n, stride=stride)
        out, dev_out, nk, after = _dev(hip, slam, rec, T)
        assert nk == len(want) and _same(out, want, f"{name} stride {stride} n {n}") and _same(dev_out, want, "*d_out")
        assert np.array_equal(after, rec)
        assert _same(slam.registered_scan(rec, T), want, f"{name} stride {stride} n {n} host entry")


@pytest.mark.parametrize("at", [4, 8, 12])
def test_stride_32_from_a_base_that_is_only_4_byte_aligned(slam, hip, at):
    """the dword instantiation on 32-byte records: equal to the aligned run"""
    for name in ("scan", "livox"):
        rec, T, want, _, _ = rr.family(name, 2 * rr.TILE + 77)
        aligned, _, nk0, _ = _dev(hip, slam, rec, T)
        out, dev_out, nk, after = _dev(hip, slam, rec, T, at=at)
        assert nk == nk0 == len(want) and _same(out, aligned, f"{name} base + {at}") and _same(dev_out, aligned, "*d_out") and _same(out, want, "want")
        assert np.array_equal(after, rec)


def test_host_entry_in_place_and_out_of_place(slam):
    for name in rr.FAMILIES:
        for n in (0, 1, 257, 3 * rr.TILE):
            rec, T, want, _, _ = rr.family(name, n)
            src = rec.copy()
            got = slam.registered_scan(src, T)
            assert _same(got, want, f"{name} {n} out of place") and np.array_equal(src, rec), "out of place: the records stay"
            buf = rec.copy()
            got = slam.registered_scan(buf, T, in_place=True)
            assert _same(got, want, f"{name} {n} in place") and got.ctypes.data == buf.ctypes.data if n else len(got) == 0
    # without an output buffer: the count alone
    rec, T, want, _, _ = rr.family("scan", 3 * rr.TILE)
    nk = C.c_size_t(0)
    Tc = np.array(T)
    assert slam.L.so_icp_registered_scan(slam.h, rec.ctypes.data_as(C.c_void_p), len(rec), 32, Tc.ctypes.data_as(C.POINTER(C.c_double)), None,
                                         C.byref(nk)) == 0 and nk.value == len(want)


def test_two_calls_in_a_row_with_different_poses(slam, hip):
    """the ticket, the count and the look-back words are cleared per call; *d_out of a call without a host copy holds the same bytes"""
    rec, T, want, _, _ = rr.family("scan", 5 * rr.TILE + 3)
    d, addr = hip.upload(rec)
    try:
        for seed in (1, 2, 1):
            T2 = rr.pose(seed)
            want2, _, keep2 = rr.registered_scan(rec, T2)
            out, d_out, nk = slam.registered_scan_dev(addr, len(rec), 32, T2)
            assert nk == len(want2) and _same(out, want2, f"pose {seed}")
            none, d_out2, nk2 = slam.registered_scan_dev(addr, len(rec), 32, T2, want_host=False)
            assert none is None and nk2 == nk and _same(hip.download(d_out2, nk * 32).reshape(nk, 32), want2, f"pose {seed} resident only")
        assert len(want2) != len(rr.registered_scan(rec, rr.pose(2))[0]) or not np.array_equal(want2, rr.registered_scan(rec, rr.pose(2))[0])
        out, d_out, nk = slam.registered_scan_dev(0, 0, 32, T)
        assert nk == 0 and len(out) == 0 and d_out is None
    finally:
        hip.free(d)


def _ouster(soicp):
    buf, w, h, rs, _ = fr.ouster_sweep(64, 48, seed=5, nan_every=97, zero_every=61)
    return buf, w, h, fr.layout_for(fr.SENSOR_OUSTER, 3, 0.2, row_step=rs)


@pytest.mark.parametrize("sensor", ["ouster", "livox"])
def test_resident_chain(gpu_slam_factory, soicp, hip, sensor):
    """extract_features(_livox)_dev -> registered_scan_dev on *d_nodistortion_out equals the restatement on the host copy of those
    records; again after prefilter_scan_dev + localization_dev on the same context: the same bytes, *d_nodistortion_out intact, and
    the first *d_out still what it was"""
    if sensor == "ouster":  # an empty map: the first localization seeds it with the sweep, as the node's first frame does
        s = gpu_slam_factory(plane_res=0.2, max_iterations=4)
        line_res, plane_res, initialized, T = 0.2, 0.4, False, rr.pose(3)
    else:
        sc = synth.Scene("mid360_like")
        s = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=4000, max_iterations=4)
        line_res, plane_res, initialized, T = sc.plane_res / 2, sc.plane_res, True, sc.guess(0)
    try:
        if sensor == "ouster":
            payload, w, h, layout = _ouster(soicp)
            n = w * h
            poses = dd.pose_buffer(T0, seed=22, translate=False)
            d, addr = hip.upload(payload)
            extract = lambda: s.extract_features_dev(addr, w, h, layout, T0, poses, True, None)  # noqa: E731
        else:
            s.add_surf_point_cloud(sc.map_points)
            vals = lr.chain_sweep(0, sc.scan(0))
            n = len(vals["x"])
            layout = soicp.livox_layout(3, 0.2, R_imu_laser_gravity=lr.R_TILT)
            poses = lr.small_motion_poses(T0, seed=90)
            d, addr = hip.upload(synth.livox_points(vals))
            extract = lambda: s.extract_features_livox_dev(addr, n, layout, T0, poses, False, None)  # noqa: E731
        try:
            d_rec, d_surf, info = extract()
            rec = hip.download(d_rec, 32 * n).reshape(n, 32)
            want, near, keep = rr.registered_scan(rec, T)
            assert 0 < len(want) < n, "the sweep has records that are dropped (zero records, NaN points)"
            out, d_out, nk = s.registered_scan_dev(d_rec, n, 32, T)
            assert nk == len(want) and _same(out, want, sensor) and _same(hip.download(d_out, nk * 32).reshape(nk, 32), want, "*d_out")
            dp, n_f, _ = s.prefilter_scan_dev(d_surf, info.n_surface, 32, 1, line_res, plane_res)
            assert _same(hip.download(d_out, nk * 32).reshape(nk, 32), want, "*d_out behind the pre-filter")
            rc, p, st = s.localization_dev(initialized, T, dp, n_f, T0)
            assert rc >= 0
            assert np.array_equal(hip.download(d_rec, 32 * n).reshape(n, 32), rec), "*d_nodistortion_out is intact"
            want2, _, _ = rr.registered_scan(rec, p)
            out2, d_out2, nk2 = s.registered_scan_dev(d_rec, n, 32, p)
            assert nk2 == len(want2) and _same(out2, want2, sensor + " at the registered pose")
            out3, d_out3, nk3 = s.registered_scan_dev(d_rec, n, 32, T)
            assert nk3 == nk and _same(out3, want, sensor + " again")
            assert np.array_equal(hip.download(d_rec, 32 * n).reshape(n, 32), rec)
            d_rec2, _, info2 = extract()
            assert _same(hip.download(d_out3, nk3 * 32).reshape(nk3, 32), want, "*d_out behind the next feature extraction")
        finally:
            hip.free(d)
    finally:
        s.close()
