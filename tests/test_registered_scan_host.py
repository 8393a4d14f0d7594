"""CPU-side checks of so_icp_registered_scan(_dev): the symbols are exported and the ABI version stays 4, every bad argument is refused
with its code on a host-only context (argument checks first, then SO_ICP_E_HIP: no CPU fallback), the numpy restatement
(tests/registered_scan_ref.py) equals a plain per-point loop, and the inputs of tests/test_gpu_registered_scan.py carry what those
tests claim to exercise.  No compute kernels run here."""
import ctypes as C

import numpy as np
import pytest

import registered_scan_ref as rr

E_INVALID, E_HIP, E_UNSUPPORTED = -1, -2, -5
NEW = ["so_icp_registered_scan", "so_icp_registered_scan_dev"]


def test_symbols_are_exported_and_the_abi_version_stays(soicp):
    L = soicp.load()
    for name in NEW:
        assert hasattr(L, name) and name in soicp.EXPORTED
    assert L.so_icp_abi_version() == 4


def test_error_codes_are_the_headers(soicp):
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "so_icp.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+SO_ICP_E_(\w+)\s+\(?(-?\d+)\)?", text)}
    assert (codes["INVALID"], codes["HIP"], codes["UNSUPPORTED"]) == (E_INVALID, E_HIP, E_UNSUPPORTED)


def _call(L, h, rec, n, stride, T, dev, out=None):
    p = None if rec is None else (C.c_void_p(rec) if isinstance(rec, int) else rec.ctypes.data_as(C.c_void_p))
    Tp = None if T is None else T.ctypes.data_as(C.POINTER(C.c_double))
    o = None if out is None else out.ctypes.data_as(C.c_void_p)
    nk = C.c_size_t(77)
    if dev:
        d = C.c_void_p()
        return L.so_icp_registered_scan_dev(h, p, n, stride, Tp, o, C.byref(d), C.byref(nk)), nk.value
    return L.so_icp_registered_scan(h, p, n, stride, Tp, o, C.byref(nk)), nk.value


@pytest.mark.parametrize("dev", [False, True])
def test_invalid_arguments_and_the_host_only_context(soicp, dev):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    n = 320
    rec, T, _, _, _ = rr.family("scan", n)
    T = np.array(T)
    out = np.zeros_like(rec)
    assert _call(L, None, rec, n, 32, T, dev)[0] == E_INVALID        # no context
    assert _call(L, host.h, rec, n, 32, None, dev)[0] == E_INVALID   # no pose
    assert _call(L, host.h, None, n, 32, T, dev)[0] == E_INVALID     # no records, n > 0
    for stride in (0, 4, 8, 11, 13, 14, 18, 30, 33):
        assert _call(L, host.h, rec, 3, stride, T, dev)[0] == E_INVALID, stride
        assert b"stride" in L.so_icp_last_error(host.h)
    assert _call(L, host.h, rec, 2**31, 32, T, dev)[0] == E_UNSUPPORTED
    assert _call(L, host.h, rec, 2**33 + 5, 12, T, dev)[0] == E_UNSUPPORTED
    if dev:  # a device address that is not 4-byte aligned (any number will do: the argument checks dereference nothing)
        for off in (1, 2, 3):
            assert _call(L, host.h, 0x7F0000001000 + off, n, 32, T, True)[0] == E_INVALID, off
            assert b"aligned" in L.so_icp_last_error(host.h)
        assert _call(L, host.h, 0x7F0000001000 + 4, n, 32, T, True)[0] == E_HIP
    # valid arguments on a host-only context: E_HIP, nothing written
    for stride in (12, 16, 20, 32, 48):
        assert _call(L, host.h, rec, n * 32 // stride // 2, stride, T, dev, out)[0] == E_HIP, stride
        assert b"host-only" in L.so_icp_last_error(host.h)
    assert _call(L, host.h, rec, n, 32, T, dev, None)[0] == E_HIP        # out is nullable
    assert _call(L, host.h, None, 0, 32, T, dev)[0] == E_HIP             # n == 0: the device check still comes before the work
    assert not out.any()


@pytest.mark.parametrize("name", rr.FAMILIES)
def test_restatement_equals_the_per_point_loop(name):
    for seed in (0, 1):
        rec, T, want, near, keep = rr.family(name, 300, seed=seed)
        loop = rr.registered_scan_loop(rec, T)
        assert loop.shape == want.shape and np.array_equal(loop, want), name
        assert len(want) == keep.sum() and rec.shape == (300, 32)
    if name != "livox":
        for stride in (12, 16, 20):
            rec, T, want, _, _ = rr.family(name, 300, stride=stride)
            assert rec.shape == (300, stride) and np.array_equal(rr.registered_scan_loop(rec, T), want)


def test_restatement_known_answers():
    T = np.array([1.0, 2.0, 3.0, 0, 0, np.sin(np.pi / 4), np.cos(np.pi / 4)])  # a quarter turn about z, then (1, 2, 3)
    xyz = np.array([[1, 0, 0], [0.05, 0.05, 0.05], [0, 0.1, 0], [-2, 1, -3], [-2.2, 1, -3], [np.nan, 1, 1], [0, 0, 0]], np.float32)
    rec = np.zeros((len(xyz), 8), np.float32)
    rec[:, :3] = xyz
    rec[:, 4] = np.arange(len(xyz)) + 10
    out, near, keep = rr.registered_scan(rec.view(np.uint8).reshape(-1, 32), T)
    assert near.tolist() == [False, True, False, False, False, False, True], "0.1 m itself is not < 0.1 m (float 0.1f * 0.1f > 0.01)"
    assert keep.tolist() == [True, False, True, False, True, False, False]
    f = out.view(np.float32)
    assert f[:, 4].tolist() == [10, 12, 14], "whole records, in order"
    assert np.allclose(f[0, :3], [1, 3, 3], atol=1e-6) and np.allclose(f[1, :3], [0.9, 2, 3], atol=1e-6)
    assert np.array_equal(rr.registered_scan_loop(rec.view(np.uint8).reshape(-1, 32), T), out)


@pytest.mark.parametrize("n", [s for s in rr.SIZES if s >= 2047])
def test_families_are_not_vacuous(n):
    """what tests/test_gpu_registered_scan.py claims of its inputs, from the restatement alone"""
    rec, T, want, near, keep = rr.family("scan", n)
    dropped_far = ~keep & ~near
    print(n, "scan: near-sensor", near.sum(), "near-origin drops", dropped_far.sum(), "kept", keep.sum())
    assert near.sum() >= 20 and dropped_far.sum() >= 20 and keep.sum() >= 0.9 * n
    assert not keep[near].any(), "an untransformed point within 0.1 m of the sensor is within 0.1 m of the origin"
    assert np.array_equal(want[:, 12:], rec[keep][:, 12:]) and rec[:, 12:].view(np.uint32).all(), "the payload words tell records apart"

    rec, T, want, near, keep = rr.family("livox", n)
    zero = ~rec.any(1)
    print(n, "livox: zero records", zero.mean(), "kept", keep.sum())
    assert zero.mean() >= 0.30 and np.array_equal(zero, near) and not keep[zero].any() and keep[~zero].all()
    assert (zero[1:] & zero[:-1]).any() and keep.sum() == (~zero).sum() >= 0.5 * n

    rec, T, want, near, keep = rr.family("nonfinite", n)
    at = rr.nonfinite_at(n)
    xyz = rec[:, :12].copy().view(np.float32).reshape(-1, 3)
    assert len(at) == 9 and [int(np.argmax(~np.isfinite(xyz[i]))) for i in at] == [0, 1, 2] * 3
    assert np.isnan(xyz[at[:3]]).sum() == 3 and (xyz[at[3:6]] == np.inf).sum() == 3 and (xyz[at[6:]] == -np.inf).sum() == 3
    assert (~np.isfinite(xyz)).any(1).sum() == 9 and (~keep[at]).sum() >= 6 and not near[at].any()
    assert np.isfinite(want[:, :12].copy().view(np.float32)).all() or keep[at].any(), "only a kept infinite point puts a non-finite value out"
    assert not np.isnan(want[:, :12].copy().view(np.float32)).any(), "a NaN is never published"

    rec, T, want, near, keep = rr.family("tiles_middle", n)
    if n > rr.TILE:
        mid = slice(rr.TILE, min(2 * rr.TILE, n))
        assert not keep[mid].any() and near[mid].sum() >= 1 and (~near[mid]).sum() >= (1 if n > rr.TILE + 1 else 0)
        assert keep[:rr.TILE].sum() > 0.9 * rr.TILE
    if n >= 3 * rr.TILE:
        assert keep[2 * rr.TILE:3 * rr.TILE].sum() > 0.9 * rr.TILE and near[rr.TILE:2 * rr.TILE].sum() == rr.TILE // 2

    rec, T, want, near, keep = rr.family("tiles_none", n)
    assert keep.all() and not near.any() and len(want) == n and not np.array_equal(want, rec)

    rec, T, want, near, keep = rr.family("tiles_ends", n)
    assert np.nonzero(keep)[0].tolist() == [0, n - 1] and len(want) == 2


@pytest.mark.parametrize("name", rr.FAMILIES)
def test_every_size_of_the_gpu_tests_can_be_generated(name):
    """every (family, n) and stride the GPU file asks for, the empty cloud included: the shapes, and the count the restatement gives"""
    for n in rr.SIZES:
        rec, T, want, near, keep = rr.family(name, n)
        assert rec.shape == (n, 32) and want.shape == (int(keep.sum()), 32) and near.shape == keep.shape == (n,)
    for stride in (() if name == "livox" else (12, 16, 20, 48)):
        for n in (0, 1, 257, 2 * rr.TILE + 77):
            rec, T, want, _, keep = rr.family(name, n, stride=stride)
            assert rec.shape == (n, stride) and want.shape == (int(keep.sum()), stride)
