"""CPU: so_icp_keep_sequence_correspondences / so_icp_sequence_correspondences / so_icp_sequence_correspondence_sums -- what can be held
without a device: the symbols and their declarations, the refusals on a host-only context (code and whole text; every export reports
valid = 0), the device-free layout of an export over entries of different sizes (reg_plan.h: ticket -> (entry, tile) over the prefix
table of tile counts, entries without a tile included; the record ranges from reported counts; the status offsets), and -- with the
Seam C host loop on the oracle -- that the runs tests/test_gpu_sequence_correspondences.py uses do what those tests need."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sequence_correspondences_data as scd
import sequence_priors_data as spd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "sequence_correspondences_host.cpp")
LIB = os.path.join(HERE, "native", "libsequence_correspondences_host.so")
HDR = os.path.join(ROOT, "superodom_amd", "csrc")
NO_DEVICE = "host-only context (device_id < 0): no compute path -- libsoicp has no CPU fallback"
U64P = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def native():
    deps = [SRC] + [os.path.join(HDR, h) for h in ("reg_plan.h", "so_math.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-fPIC", "-shared", "-I", HDR, SRC, "-o", LIB])
    L = C.CDLL(LIB)
    i32p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    L.sc_ticket.argtypes = [C.c_uint32, u32p, C.c_uint32, u32p]; L.sc_ticket.restype = None
    L.sc_status_ranges.argtypes = [C.POINTER(C.c_size_t), i32p, C.c_int, U64P]; L.sc_status_ranges.restype = C.c_uint64
    L.sc_selection_first_bad.argtypes = [i32p, C.c_int, C.c_int]
    L.sc_record_ranges.argtypes = [u32p, C.POINTER(C.c_uint8), i32p, C.c_int, U64P]; L.sc_record_ranges.restype = C.c_uint64
    return L


def test_symbols_and_declarations(soicp):
    L = soicp.load()
    names = ["so_icp_keep_sequence_correspondences", "so_icp_sequence_correspondences", "so_icp_sequence_correspondence_sums"]
    for name in names:
        assert name in soicp.EXPORTED and getattr(L, name)
    header = open(os.path.join(ROOT, "include", "so_icp.h")).read()
    assert re.search(r"int so_icp_keep_sequence_correspondences\(so_icp_ctx \*ctx, int on\);", header)
    assert re.search(r"int so_icp_sequence_correspondences\(so_icp_ctx \*ctx, const int32_t \*frames[^)]*int n_sel,\s*const double \*poses[^)]*"
                     r"so_icp_correspondence \*records, size_t cap_records,\s*uint64_t \*first_record[^)]*uint8_t \*status_out, size_t cap_status,\s*"
                     r"uint64_t \*first_status[^)]*void \*\*d_records_out, so_icp_correspondence_info \*info[^)]*\);", header)
    assert re.search(r"int so_icp_sequence_correspondence_sums\(so_icp_ctx \*ctx, const int32_t \*frames, int n_sel,\s*const double \*poses[^)]*"
                     r"int n_poses[^)]*so_icp_sums \*sums_out[^)]*\);", header)
    assert header.index("so_icp_batch_correspondence_sums(so_icp_ctx") < header.index("so_icp_keep_sequence_correspondences(so_icp_ctx") \
        < header.index("so_icp_sequence_correspondences(so_icp_ctx") < header.index("so_icp_sequence_correspondence_sums(so_icp_ctx")
    m = re.search(r"#define SO_ICP_SEQUENCE_MAX_SELECTION (\d+)", header)
    assert m and int(m.group(1)) == soicp.SEQUENCE_MAX_SELECTION == 1024
    assert L.so_icp_abi_version() == 4  # (no version bump: no struct changed)
    for method in ("keep_sequence_correspondences", "sequence_correspondences", "sequence_correspondence_sums"):
        assert hasattr(soicp.LidarSlamGpu, method)
    section = header[header.index("the correspondence sets of a RUN's frames"):header.index("so_icp_keep_sequence_correspondences(so_icp_ctx")]
    assert "LS.h:209-222" in section and "53 bytes per point and frame" in section


def test_host_only_context_refusals_and_nothing_to_export(soicp):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    err = lambda: L.so_icp_last_error(host.h).decode()
    # the switch
    assert L.so_icp_keep_sequence_correspondences(None, 1) == -1
    for on in (1, 0):
        assert L.so_icp_keep_sequence_correspondences(host.h, on) == -2 and err() == NO_DEVICE
    assert host.keep_sequence_correspondences(True) == -2
    # the export: refused, and every entry reports valid = 0 with zero counts, ranges and offsets
    n_sel = 3
    info = (soicp.CorrespondenceInfo * n_sel)()
    C.memset(info, 0xFF, C.sizeof(info))
    first = np.full(n_sel + 1, 7, np.uint64); first_status = np.full(n_sel + 1, 9, np.uint64)
    d = C.c_void_p(1)
    assert L.so_icp_sequence_correspondences(None, None, n_sel, None, None, 0, None, None, 0, None, None, None) == -1
    rc = L.so_icp_sequence_correspondences(host.h, None, n_sel, None, None, 0, first.ctypes.data_as(U64P), None, 0, first_status.ctypes.data_as(U64P), C.byref(d), info)
    assert rc == -2 and err() == NO_DEVICE
    assert bytes(info) == bytes(C.sizeof(info)) and not first.any() and not first_status.any() and d.value is None
    for bad in (-1, soicp.SEQUENCE_MAX_SELECTION + 1):
        assert L.so_icp_sequence_correspondences(host.h, None, bad, None, None, 0, None, None, 0, None, None, None) == -1
        assert err() == "so_icp_sequence_correspondences: n_sel must be 0 .. SO_ICP_SEQUENCE_MAX_SELECTION"
    with pytest.raises(soicp.SoIcpError) as e:
        host.sequence_correspondences(n_sel=2)
    assert str(e.value) == "so_icp error -2: " + NO_DEVICE
    # the sums: argument checks first, then the refusal; the output is zeroed
    poses = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (n_sel, 2, 1))
    pp = poses.ctypes.data_as(C.POINTER(C.c_double))
    out = (soicp.Sums * (n_sel * 2))()
    C.memset(out, 0xFF, C.sizeof(out))
    assert L.so_icp_sequence_correspondence_sums(None, None, n_sel, pp, 2, out) == -1
    assert L.so_icp_sequence_correspondence_sums(host.h, None, n_sel, pp, 2, out) == -2 and err() == NO_DEVICE
    assert bytes(out) == bytes(C.sizeof(out))
    for n_poses in (0, soicp.SUMS_MAX_POSES + 1):
        assert L.so_icp_sequence_correspondence_sums(host.h, None, n_sel, pp, n_poses, out) == -1
        assert err() == "so_icp_sequence_correspondence_sums: n_poses must be 1 .. SO_ICP_SUMS_MAX_POSES"
    for bad in (-1, soicp.SEQUENCE_MAX_SELECTION + 1):
        assert L.so_icp_sequence_correspondence_sums(host.h, None, bad, pp, 2, out) == -1
        assert err() == "so_icp_sequence_correspondence_sums: n_sel must be 0 .. SO_ICP_SEQUENCE_MAX_SELECTION"
    for a, b in ((None, out), (pp, None)):
        assert L.so_icp_sequence_correspondence_sums(host.h, None, n_sel, a, 2, b) == -1
        assert err() == "so_icp_sequence_correspondence_sums: poses and sums_out must not be NULL"
    with pytest.raises(soicp.SoIcpError) as e:
        host.sequence_correspondence_sums(poses)
    assert str(e.value) == "so_icp error -2: " + NO_DEVICE
    host.close()


def _tickets(native, tiles):
    """every ticket of a selection whose entries have `tiles` tiles -> [(entry, tile)]"""
    first = np.concatenate([[0], np.cumsum(tiles)]).astype(np.uint32)
    out = (C.c_uint32 * 2)()
    got = []
    for t in range(int(first[-1])):
        native.sc_ticket(t, first.ctypes.data_as(C.POINTER(C.c_uint32)), len(tiles), out)
        got.append((out[0], out[1]))
    return first, got


@pytest.mark.parametrize("tiles", [[1], [3], [1, 0, 3, 0, 0, 2], [0, 0, 1], [2, 0], [0, 5, 0], [1, 1, 1, 1], [4, 1, 2, 7, 1], [0, 0, 0, 0],
                                   [1] * 1024, [0] * 1000 + [3] + [0] * 23, [(n + scd.TILE - 1) // scd.TILE for n in scd.SIZES]])
def test_every_ticket_of_small_selections(native, tiles):
    """entry-major: the tickets of entry k are tile_first[k] .. tile_first[k + 1] - 1, tile after tile, and an entry without tiles gets
    none -- so a workgroup's look-back (tiles below its own, same entry) only ever names smaller tickets, and every (entry, tile) is
    worked on exactly once"""
    first, got = _tickets(native, tiles)
    assert got == [(k, b) for k in range(len(tiles)) for b in range(tiles[k])]
    assert len(got) == sum(tiles)
    for t, (k, tile) in enumerate(got):
        assert (k, tile) == scd.ticket_ref(t, first)
        assert tiles[k] > 0 and all(int(first[k]) + below < t for below in range(tile)), "a predecessor of the chain with a larger ticket"
    if not any(tiles):
        assert got == [], "a selection of only empty entries launches nothing"


def test_status_offsets_and_record_ranges(native):
    n_points = [2049, 1, 0, 1025, 63]
    def status(frames, n_sel=None):
        n_sel = len(frames) if frames is not None else n_sel
        f = None if frames is None else (C.c_int32 * max(1, n_sel))(*frames)
        first = (C.c_uint64 * (n_sel + 1))(*([99] * (n_sel + 1)))
        total = native.sc_status_ranges((C.c_size_t * len(n_points))(*n_points), f, n_sel, first)
        return total, list(first)
    # a row is as long as its frame, valid or not; an empty frame has an empty row
    assert status(None, 5) == (3138, [0, 2049, 2050, 2050, 3075, 3138])
    assert status(None, 0) == (0, [0]) and status([2]) == (0, [0, 0])
    assert status([4, 0, 0, 2, 3]) == (63 + 2 * 2049 + 1025, [0, 63, 2112, 4161, 4161, 5186])
    # the record ranges: batch_record_ranges' arithmetic on the counts the frames reported
    accepted, valid = [1500, 1, 0, 900, 40], [1, 1, 1, 0, 1]
    def ranges(frames, n_sel=None):
        n_sel = len(frames) if frames is not None else n_sel
        f = None if frames is None else (C.c_int32 * max(1, n_sel))(*frames)
        first = (C.c_uint64 * (n_sel + 1))(*([99] * (n_sel + 1)))
        total = native.sc_record_ranges((C.c_uint32 * 5)(*accepted), (C.c_uint8 * 5)(*valid), f, n_sel, first)
        return total, list(first)
    assert ranges(None, 5) == (1541, [0, 1500, 1501, 1501, 1501, 1541])  # (frame 3 stopped the run: it has no records whatever it counted)
    assert ranges([4, 3, 0, 0]) == (3040, [0, 40, 40, 1540, 3040])
    bad = lambda frames, n: native.sc_selection_first_bad((C.c_int32 * max(1, len(frames)))(*frames), len(frames), n)
    assert bad([0, 4, 4, 2], 5) == -1 and bad([0, 5], 5) == 1 and bad([-1], 5) == 0


def test_reg_plan_still_needs_no_device_headers():
    text = open(os.path.join(HDR, "reg_plan.h")).read()
    assert sorted(re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)) == ["algorithm", "cstddef", "cstdint", "so_math.h"]
    assert "selection_ticket" in text and "sequence_status_ranges" in text


def test_the_runs():
    assert scd.SIZES == [2049, 0, 1025, 1, 63, 64, 65, 255, 256, 257, 1023, 1024]
    assert sorted(scd.SIZES) == [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
    sc, scans, pose0, deltas, priors, modes = scd.run_inputs("sizes")
    assert [len(s) for s in scans] == scd.SIZES and deltas.shape == (12, 7) and priors is None
    tiles = [int(t) for t in np.diff(scd.tile_first(scd.SIZES))]
    assert tiles == [3, 0, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1], "unequal tile counts, a zero-tile entry in the middle"
    assert [scd.SIZES[f] for f in scd.SUMS_FRAMES] == [1, 255, 1024, 1025, 2049]
    sc, scans, pose0, deltas, priors, modes = scd.run_inputs("sizes_chained")
    assert [len(s) for s in scans] == scd.SIZES_CHAINED == [2049, 1025, 64, 65, 255] and deltas.shape == (5, 7)
    assert [int(t) for t in np.diff(scd.tile_first(scd.SIZES_CHAINED))] == [3, 2, 1, 1, 1]
    for run in scd.PLAIN_RUNS:
        assert scd.run_inputs(run)[4] is None
    sc, scans, pose0, deltas, priors, modes = scd.run_inputs("broken")
    assert modes == [spd.AT_GUESS] * len(scans) and len(priors) == len(scans)


@pytest.mark.parametrize("run", scd.PLAIN_RUNS + ("broken",))
def test_the_runs_do_what_the_gpu_tests_need(oracle, run):
    """On the oracle, through the Seam C host loop, chained as the entry chains: every frame accepts points, the frames accept
    different point sets (an export that read another frame's slice could not pass the GPU tests) and do not all end in the same outer
    iteration; by the schedule restated on iteration counts (sequence_priors_data.schedule) the chunked run has chained frames and the
    broken run breaks its chain."""
    rows = scd.oracle_frames(oracle, run)
    iters = [r[0] for r in rows]
    if run == "broken":
        assert iters == spd.oracle_iterations(oracle, run, scd.PRIOR_KIND), "the same loop as sequence_priors_data's"
    chained, breaks = spd.schedule(iters)
    print(run, "outer iterations", iters, "accepted", [len(r[1]) for r in rows], "chained", chained, "breaks", breaks)
    assert all(len(r[1]) >= 1 for r in rows)
    assert len({r[1].tobytes() for r in rows}) == len(rows), "two frames accept the same points"
    assert len(set(iters)) >= 2, "every frame ends in the same outer iteration"
    if run == "small_chunked":
        assert sum(chained) >= 2
    if run == "broken":
        assert breaks >= 1
