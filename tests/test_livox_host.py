"""CPU-side checks of so_icp_extract_features_livox(_dev): the symbols are exported and the ABI version stays 4, the ctypes mirror of
so_icp_livox_layout has the C compiler's size and offsets, a host-only context fails with SO_ICP_E_HIP, every bad layout is refused with
SO_ICP_E_INVALID and a message that names the field, livox_ros_driver2/msg/CustomMsg passes adapter/wire_selftest byte for byte, and
the sweeps of tests/test_gpu_livox.py carry what those tests claim to exercise.  No compute kernels run here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import livox_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "adapter", "wire_selftest")
E_INVALID, E_HIP = -1, -2
NEW = ["so_icp_livox_default_layout", "so_icp_extract_features_livox", "so_icp_extract_features_livox_dev"]


def test_symbols_are_exported_and_the_abi_version_stays(soicp):
    L = soicp.load()
    for name in NEW:
        assert hasattr(L, name) and name in soicp.EXPORTED
    assert L.so_icp_abi_version() == 4


def test_layout_mirror_matches_the_c_struct(soicp, tmp_path):
    fields = [f for f, _ in soicp.LivoxLayout._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "so_icp.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(so_icp_livox_layout));\n'
                   + "".join(f'  printf(" %zu", offsetof(so_icp_livox_layout, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(soicp.LivoxLayout) == 120
    assert got[1:] == [getattr(soicp.LivoxLayout, f).offset for f in fields]


def test_default_layout_is_the_custom_point(soicp):
    L = soicp.livox_layout()
    assert (L.point_step, L.off_offset_time, L.off_x, L.off_y, L.off_z, L.off_reflectivity, L.off_tag, L.off_line) == (20, 0, 4, 8, 12, 16, 17, 18)
    assert (L.n_scans, L.filter_point_size) == (4, 3) and L.min_range == np.float32(0.2) and L.reserved == 0
    assert list(L.R_imu_laser_gravity) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    M = soicp.livox_layout(7, 0.5, n_scans=6, R_imu_laser_gravity=lr.R_TILT, point_step=24, offsets={"line": 23, "offset_time": 16, "reflectivity": 0})
    assert (M.point_step, M.off_line, M.off_offset_time, M.off_reflectivity, M.n_scans, M.filter_point_size) == (24, 23, 16, 0, 6, 7)
    assert np.array_equal(np.array(M.R_imu_laser_gravity[:]), lr.R_TILT.reshape(9))


def _call(L, h, layout, buf, n, poses=None, dev=False, n_poses=None):
    n_poses = (0 if poses is None else len(poses)) if n_poses is None else n_poses
    pp = None if poses is None else poses.ctypes.data_as(C.POINTER(C.c_double))
    from superodom_amd.binding import FeatureInfo
    info = FeatureInfo()
    raw = None if buf is None else buf.ctypes.data_as(C.c_void_p)
    lay = None if layout is None else C.byref(layout)
    if dev:
        d_rec, d_surf = C.c_void_p(), C.c_void_p()
        return L.so_icp_extract_features_livox_dev(h, raw, n, lay, 0.0, pp, n_poses, 0, None, C.byref(d_rec), C.byref(d_surf), C.byref(info))
    return L.so_icp_extract_features_livox(h, raw, n, lay, 0.0, pp, n_poses, 0, None, None, None, C.byref(info))


@pytest.mark.parametrize("dev", [False, True])
def test_invalid_arguments_and_the_host_only_context(soicp, dev):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    n = 320
    from superodom_amd import synth
    buf = synth.livox_points(synth.livox_sweep(n=n, seed=1))
    good = soicp.livox_layout()
    assert _call(L, None, good, buf, n, dev=dev) == E_INVALID        # no context
    assert _call(L, host.h, None, buf, n, dev=dev) == E_INVALID      # no layout
    assert _call(L, host.h, good, None, n, dev=dev) == E_INVALID     # no payload
    assert _call(L, host.h, good, buf, n, n_poses=3, dev=dev) == E_INVALID  # n_poses without a buffer

    def bad(word, **kw):
        lay = soicp.livox_layout()
        for k, v in kw.items():
            setattr(lay, k, v)
        assert _call(L, host.h, lay, buf, n, dev=dev) == E_INVALID, kw
        msg = L.so_icp_last_error(host.h)
        assert word.encode() in msg, (kw, msg)
    bad("offset_time", off_offset_time=17)     # 4 bytes at 17 run past point_step 20
    bad("offset of x", off_x=20)
    bad("offset of y", off_y=-1)               # a CustomPoint has every field: no "absent"
    bad("offset of z", off_z=18)
    bad("reflectivity", off_reflectivity=20)
    bad("tag", off_tag=-2)
    bad("line", off_line=20)
    bad("line", point_step=18)                 # point_step in front of the end of the last field
    bad("point_step", point_step=0)
    bad("filter_point_size", filter_point_size=0)
    bad("filter_point_size", filter_point_size=-3)
    bad("n_scans", n_scans=-1)
    bad("n_scans", n_scans=257)
    for ok in (dict(n_scans=0), dict(n_scans=256), dict(point_step=19), dict(off_line=0, off_offset_time=1, off_x=5, off_y=9, off_z=13, off_reflectivity=17, off_tag=18)):
        lay = soicp.livox_layout()
        for k, v in ok.items():
            setattr(lay, k, v)
        assert _call(L, host.h, lay, buf, n, dev=dev) == E_HIP, ok  # a valid layout gets as far as the device check
    # a valid call on a host-only context: E_HIP, nothing touched; n == 0 included (the device check comes before the work)
    poses = np.zeros((3, 8))
    assert _call(L, host.h, good, buf, n, poses=poses, dev=dev) == E_HIP
    assert b"host-only" in L.so_icp_last_error(host.h)
    assert host.export_map().size == 0


def _selftest(*args):
    subprocess.check_call([SELFTEST] + [str(a) for a in args])


def test_custom_msg_roundtrip_through_the_cpp_codec(tmp_path):
    """Python writer -> wire_selftest roundtrip CustomMsg -> identical bytes; elements 20 bytes apart, none behind the last"""
    from superodom_amd import synth
    for n, frame in ((0, ""), (1, "a"), (5, "livox_frame"), (257, "abcd")):
        vals = synth.livox_sweep(n=max(n, 2), seed=5 + n)
        vals = {k: v[:n] for k, v in vals.items()}
        raw = lr.encode_custom_msg(lr.custom_msg(vals, frame_id=frame))
        at, point_num, count = lr.points_in_cdr(raw)
        assert point_num == count == n and len(raw) == at + (20 * n - 1 if n else 0), "19-byte elements aligned to 4, no padding after the last"
        if n:
            assert bytes(raw[at:]) == synth.livox_points(vals).tobytes(), "the sequence's bytes are the payload the library takes"
        src, dst = tmp_path / f"in{n}.cdr", tmp_path / f"out{n}.cdr"
        src.write_bytes(raw)
        _selftest("roundtrip", "CustomMsg", src, dst)
        assert dst.read_bytes() == raw
    # truncated in the middle of the last point: refused
    src.write_bytes(raw[:-3])
    assert subprocess.run([SELFTEST, "roundtrip", "CustomMsg", str(src), str(dst)], capture_output=True).returncode == 1


def test_custom_msg_emitted_by_the_cpp_codec_parses(tmp_path):
    """wire_selftest emit CustomMsg with frame_ids of length 0 .. 8: the padding in front of the uint64 timebase takes every value it
    can, and the Python reader finds the fields the C++ side wrote.  (CDR aligns timebase to 8 and the element count to 4, so inside
    the message the points always start on a multiple of 4 -- asserted; the alignments 1 .. 3 of a payload in memory are the business of
    tests/test_gpu_livox.py::test_unaligned_and_packed_payloads.)"""
    pads = set()
    for k in range(9):
        frame = "livox_frame"[:k]
        out = tmp_path / f"emit{k}.cdr"
        _selftest("emit", "CustomMsg", out, frame)
        raw = out.read_bytes()
        m = lr.decode_custom_msg(raw)
        assert m["header"] == {"stamp": {"sec": 1700000000, "nanosec": 250000000}, "frame_id": frame}
        assert (m["timebase"], m["point_num"], m["lidar_id"], m["rsvd"]) == (1700000000250000000, 5, 192, [1, 2, 3])
        assert m["points"] == [{"offset_time": 20000 * i + 7, "x": 1.5 * i, "y": -0.25 * i, "z": 0.125 + i, "reflectivity": 10 * i,
                                "tag": 0x10 * i, "line": i % 4} for i in range(5)]
        at, _, count = lr.points_in_cdr(raw)
        assert (at - 4) % 4 == 0 and count == 5 and len(raw) == at + 99
        end_of_frame = 4 + 8 + 4 + k + 1
        pads.add(at - 20 - end_of_frame)  # timebase, point_num, lidar_id + rsvd, count: 20 bytes in front of the points
        assert raw == lr.encode_custom_msg(m)
    assert pads == set(range(8)), pads
    _selftest("emit", "CustomMsg", tmp_path / "default.cdr")
    assert lr.decode_custom_msg((tmp_path / "default.cdr").read_bytes())["header"]["frame_id"] == "livox_frame"


def test_restatement_known_answers():
    vals = {"offset_time": np.array([0, 1, 999999999, 50000000, 7], np.uint32), "x": np.array([1, 2, 3, 4, np.inf], np.float32),
            "y": np.array([0.5, 0, 0, 0, 1], np.float32), "z": np.array([0, 0, 0, 0, 2], np.float32),
            "reflectivity": np.array([0, 255, 7, 9, 1], np.uint8), "tag": np.array([0x00, 0x1F, 0x20, 0xC0, 0x10], np.uint8),
            "line": np.array([0, 3, 1, 4, 2], np.uint8)}
    assert lr.accepted(vals).tolist() == [True, True, False, False, True]  # 0x20: tag; line 4: not < N_SCANS
    assert lr.accepted(vals, n_scans=5).tolist() == [True, True, False, True, True] and not lr.accepted(vals, n_scans=0).any()
    rec = lr.ingest(vals)
    f, u = rec.view(np.float32), rec.view(np.uint32)
    assert not rec[2].any() and not rec[3].any(), "a rejected point is the value-initialised record"
    assert f[0].tolist() == [1, 0.5, 0, 0, 0, 0, 0, 0] and u[1, 6] == 3 and f[1, 4] == 255.0 and not u[:, [3, 7]].any()
    assert f[1, 5] == np.float32(1.0) / np.float32(1e9)
    assert f[4, 0] == np.inf and np.isnan(f[4, 1]) and np.isnan(f[4, 2]), "the identity is multiplied too: 0 * inf"
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    assert lr.ingest(vals, Rz).view(np.float32)[0, :3].tolist() == [-0.5, 1, 0]
    raw = np.frombuffer(lr.encode_custom_msg(lr.custom_msg(vals)), np.uint8)
    back = lr.values_of_points(raw[lr.points_in_cdr(raw)[0]:], 5)
    assert all(np.array_equal(back[k].view(np.uint8), vals[k].view(np.uint8)) for k in vals)


@pytest.mark.parametrize("name", list(lr.GPU_SWEEPS) + ["chain0", "chain1", "chain2"])
def test_gpu_sweeps_are_not_vacuous(name):
    """every sweep tests/test_gpu_livox.py uses: >= 1 % of the points rejected by tag and >= 1 by line, >= 80 % accepted, and
    >= 20 % of the offsets with t / 1e9f != t * 1e-9f"""
    vals = lr.chain_sweep(int(name[5:])) if name.startswith("chain") else lr.gpu_sweep(name)
    n = len(vals["x"])
    by_tag = (vals["tag"] & 0x30) >= 0x20
    by_line = vals["line"] >= 4
    differ = lr.time_div(vals["offset_time"]) != lr.time_mul(vals["offset_time"])
    print(name, n, by_tag.mean(), by_line.sum(), lr.accepted(vals).mean(), differ.mean())
    assert by_tag.mean() >= 0.01 and by_line.sum() >= 1 and lr.accepted(vals).mean() >= 0.8 and differ.mean() >= 0.2
    assert 0 < vals["offset_time"].max() < 100_000_000 and (np.diff(vals["offset_time"].astype(np.int64)) >= 0).all(), "spread over 100 ms"
    assert sorted(set(vals["line"][lr.accepted(vals)].tolist())) == [0, 1, 2, 3]
    acc = lr.accepted(vals)
    assert (~acc[1:] & ~acc[:-1]).any() and (~acc[1:] & acc[:-1]).any(), "zero records behind zero records and behind points: both sampler outcomes"
