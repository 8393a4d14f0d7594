"""CPU-side checks of so_icp_extract_features_untimed(_dev) -- featureExtraction::assignTimeforPointCloud, the ingest of a sweep without
per-point time -- and of its restatement tests/untimed_ref.py: the symbols are exported and the ABI version stays 4, the ctypes mirror
has the C compiler's layout, bad arguments are refused; the literal loop and the prefix rule agree; the ring tables are right on both
sides of every ring boundary; the NaN rule; the time column against exact rational arithmetic; the host build of the kernel's own
arithmetic header (csrc/untimed_math.h) gives the restatement's bits, and its device build holds the correctly rounded square root
and quotient; and every sweep of tests/test_gpu_untimed.py is 100 % decided
and carries what those tests claim to exercise.  No compute kernels run here."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import untimed_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_HIP = -1, -2
NEW = ["so_icp_extract_features_untimed", "so_icp_extract_features_untimed_dev"]
F32 = np.float32


def test_symbols_are_exported_and_the_abi_version_stays(soicp):
    L = soicp.load()
    for name in NEW:
        assert hasattr(L, name) and name in soicp.EXPORTED
    assert L.so_icp_abi_version() == 4


def test_layout_mirror_matches_the_c_struct(soicp, tmp_path):
    fields = [f for f, _ in soicp.UntimedLayout._fields_]
    assert fields == ["is_bigendian", "point_step", "row_step", "off_x", "off_y", "off_z", "off_intensity", "n_scans", "filter_point_size", "min_range"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "so_icp.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(so_icp_untimed_layout));\n'
                   + "".join(f'  printf(" %zu", offsetof(so_icp_untimed_layout, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(soicp.UntimedLayout) == 40
    assert got[1:] == [getattr(soicp.UntimedLayout, f).offset for f in fields]


def test_layout_from_point_fields(soicp):
    L = soicp.untimed_layout(ur.XYZI_RING_18, 18, 18 * 7, 16, 3, 0.2)
    assert (L.is_bigendian, L.point_step, L.row_step, L.off_x, L.off_y, L.off_z, L.off_intensity) == (0, 18, 126, 0, 4, 8, 12)
    assert (L.n_scans, L.filter_point_size) == (16, 3) and L.min_range == F32(0.2)
    M = soicp.untimed_layout([("x", 0, soicp.FLOAT32, 1), ("y", 4, soicp.FLOAT64, 1), ("z", 12, soicp.FLOAT32, 3), ("intensity", 24, soicp.FLOAT32, 0)],
                             28, 28, 64, 1, 0.5, is_bigendian=True)
    assert (M.is_bigendian, M.off_x, M.off_y, M.off_z, M.off_intensity) == (1, 0, -1, -1, 24), "datatype and count have to match, as in sweep_layout"


def _call(L, h, layout, buf, width, height=1, poses=None, dev=False, n_poses=None):
    from superodom_amd.binding import FeatureInfo
    n_poses = (0 if poses is None else len(poses)) if n_poses is None else n_poses
    pp = None if poses is None else poses.ctypes.data_as(C.POINTER(C.c_double))
    info = FeatureInfo()
    raw = None if buf is None else buf.ctypes.data_as(C.c_void_p)
    lay = None if layout is None else C.byref(layout)
    if dev:
        d_rec, d_surf = C.c_void_p(), C.c_void_p()
        return L.so_icp_extract_features_untimed_dev(h, raw, width, height, lay, 0.0, pp, n_poses, 0, None, C.byref(d_rec), C.byref(d_surf), C.byref(info))
    return L.so_icp_extract_features_untimed(h, raw, width, height, lay, 0.0, pp, n_poses, 0, None, None, None, C.byref(info))


@pytest.mark.parametrize("dev", [False, True])
def test_invalid_arguments_and_the_host_only_context(soicp, dev):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    n = 320
    buf, width, height, row_step = ur.payload(ur.sweep(n, 16, seed=1))

    def layout(**kw):
        lay = soicp.untimed_layout(ur.XYZI, 16, row_step, 16, 3, 0.2)
        for k, v in kw.items():
            setattr(lay, k, v)
        return lay
    good = layout()
    assert _call(L, None, good, buf, n, dev=dev) == E_INVALID        # no context
    assert _call(L, host.h, None, buf, n, dev=dev) == E_INVALID      # no layout
    assert _call(L, host.h, good, None, n, dev=dev) == E_INVALID     # no payload
    assert _call(L, host.h, good, buf, n, n_poses=3, dev=dev) == E_INVALID  # n_poses without a buffer

    def bad(word, **kw):
        assert _call(L, host.h, layout(**kw), buf, n, dev=dev) == E_INVALID, kw
        msg = L.so_icp_last_error(host.h)
        assert word.encode() in msg, (kw, msg)
    for v in (0, -16, 1, 8, 15, 17, 48, 65, 127, 256):
        bad("n_scans", n_scans=v)                  # the node refuses them at start-up (featureExtraction.cpp:62)
    bad("filter_point_size", filter_point_size=0)
    bad("filter_point_size", filter_point_size=-3)
    bad("big-endian", is_bigendian=1)
    bad("point_step", point_step=0)
    bad("row_step", row_step=16 * n - 1)
    bad("offset of x", off_x=13)
    bad("offset of y", off_y=-2)
    bad("offset of z", off_z=16)
    bad("intensity", off_intensity=14)
    for ok in [dict(n_scans=v) for v in ur.N_SCANS] + [dict(off_intensity=-1), dict(off_x=-1, off_y=-1, off_z=-1), dict(row_step=16 * n + 5)]:
        assert _call(L, host.h, layout(**ok), buf, n, dev=dev) == E_HIP, ok  # a valid layout gets as far as the device check
    assert _call(L, host.h, good, buf, n, poses=np.zeros((3, 8)), dev=dev) == E_HIP
    assert b"host-only" in L.so_icp_last_error(host.h)
    assert host.export_map().size == 0


# ---- the loop bound: the literal loop against the prefix rule ----
def _both(drop):
    drop = np.asarray(drop, bool)
    n = len(drop)
    v = np.arange(n, dtype=F32)
    lit, k_lit = ur.ingest_literal(v, v, v, v, 16, drop=drop)
    vec, k_vec = ur.ingest(v, v, v, v, 16, drop=drop)
    assert np.array_equal(k_lit, k_vec) and np.array_equal(lit, vec), drop.astype(int)
    return k_vec


def test_the_two_forms_agree_on_hand_built_patterns():
    z = np.zeros
    assert _both(z(0, bool)).tolist() == []
    assert _both(z(7, bool)).tolist() == list(range(7)), "no drop"
    first = z(7, bool); first[0] = True
    assert _both(first).tolist() == [1, 2, 3, 4, 5], "the first point dropped: the last one is cut off as well"
    assert _both(np.ones(9, bool)).tolist() == [], "all dropped"
    assert _both(np.ones(1, bool)).tolist() == []
    tail = z(10, bool); tail[1] = tail[2] = True; tail[8] = tail[9] = True
    assert _both(tail).tolist() == [0, 3, 4, 5, 6, 7], "drops in the tail that is cut off anyway do not cut any further"
    only_tail = z(10, bool); only_tail[9] = True
    assert _both(only_tail).tolist() == list(range(9))
    # a cut that ends exactly at a drop: n = 8, drops at 1 and 5 -> D(5) = 1, 5 + 1 < 8 visited and dropped, then 6 + 2 = 8: not visited
    at_drop = z(8, bool); at_drop[1] = at_drop[5] = True
    assert _both(at_drop).tolist() == [0, 2, 3, 4]
    # and one where the last visited index is itself a drop whose own decrement ends the loop
    last = z(6, bool); last[0] = last[1] = last[3] = True
    assert _both(last).tolist() == [2]


def test_the_two_forms_agree_on_random_patterns():
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(0, 60))
        k = _both(rng.random(n) < rng.choice([0.02, 0.2, 0.5, 0.9]))
        assert len(k) <= n
    for n_scans in (16, 32, 64, 4):  # and through the ring arithmetic itself
        v = ur.sweep(700, n_scans, seed=9 + n_scans, drop_share=0.15)
        lit, k_lit = ur.ingest_literal(v["x"], v["y"], v["z"], v["intensity"], n_scans)
        vec, k_vec = ur.ingest(v["x"], v["y"], v["z"], v["intensity"], n_scans)
        assert np.array_equal(k_lit, k_vec) and np.array_equal(lit, vec) and (n_scans == 4 or 0 < len(k_vec) < 700)


# ---- the ring tables ----
def _expected(el, n_scans):
    """ring (None = dropped) of an elevation in degrees, in Python's double arithmetic"""
    if n_scans == 16:
        r = int((el + 15) / 2 + 0.5)
        return None if r > 15 or r < 0 else r
    if n_scans == 32:
        r = int((el + 92.0 / 3.0) * 3.0 / 4.0)
        return None if r > 31 or r < 0 else r
    r = int((2 - el) * 3.0 + 0.5) if el >= -8.83 else 32 + int((-8.83 - el) * 2.0 + 0.5)
    return None if el > 2 or el < -24.33 or r > 50 or r < 0 else r


def _boundaries(n_scans):
    if n_scans == 16:
        return [2.0 * k - 14.0 for k in range(0, 16)] + [-18.0, -17.0, -16.0]
    if n_scans == 32:
        return [4.0 * k / 3.0 - 92.0 / 3.0 for k in range(-1, 33)]
    return [2.0 - (k - 0.5) / 3.0 for k in range(1, 33)] + [-8.83 - (k - 0.5) / 2.0 for k in range(1, 21)] + [2.0, -8.83, -24.33]


def _at_elevation(el, r=10.0, az=0.3):
    e = np.deg2rad(np.asarray(el, np.float64))
    return [(r * np.cos(e) * np.cos(az)).astype(F32), (r * np.cos(e) * np.sin(az)).astype(F32), (r * np.sin(e)).astype(F32)]


@pytest.mark.parametrize("n_scans", [16, 32, 64])
def test_ring_tables_on_both_sides_of_every_boundary(n_scans):
    """1e-3 degrees either side: about 500 times what one ulp of the float atan moves the angle"""
    b = np.array(_boundaries(n_scans))
    el = np.concatenate([b - 1e-3, b + 1e-3])
    x, y, z = _at_elevation(el)
    assert ur.decided(x, y, z, n_scans).all()
    rid, drop = ur.ring(ur.angle(x, y, z), n_scans)
    want = [_expected(float(e), n_scans) for e in el]
    assert [None if d else int(r) for r, d in zip(rid, drop)] == want
    assert len({w for w in want if w is not None}) == {16: 16, 32: 32, 64: 51}[n_scans], "every ring of the table is reached"
    assert sum(w is None for w in want) >= 2


def test_ring_table_corners():
    def one(el, n_scans):
        rid, drop = ur.ring(ur.angle(*_at_elevation([el])), n_scans)
        return None if drop[0] else int(rid[0])
    assert one(-17.0, 16) == 0 and one(-17.999, 16) == 0, "int() truncates toward zero: (-1, 0) is ring 0"
    assert one(-18.001, 16) is None and one(15.999, 16) == 15 and one(16.001, 16) is None
    assert one(-31.9, 32) == 0 and one(-32.001, 32) is None and one(11.999, 32) == 31 and one(12.001, 32) is None
    assert one(1.999, 64) == 0 and one(2.001, 64) is None, "the gate at 2 degrees"
    assert one(-8.829, 64) == 32 and one(-8.831, 64) == 32, "both branches meet in ring 32 at -8.83"
    assert one(-18.079, 64) == 50 and one(-18.081, 64) is None, "rings above 50 are dropped"
    assert one(-24.329, 64) is None and one(-24.331, 64) is None, "the gate at -24.33 lies inside what ring > 50 drops already"
    for s in (4, 128):
        assert [one(e, s) for e in (-89.0, -18.5, 0.0, 45.0)] == [0, 0, 0, 0], "the wrong-scan-number branch: ring 0, nothing dropped"


def test_nan_rule_and_infinite_coordinates():
    inf, nan = np.inf, np.nan
    pts = {"origin": (0, 0, 0), "xnan": (nan, 1, 1), "ynan": (1, nan, 1), "znan": (1, 1, nan), "x+inf": (inf, 1, 1), "x-inf": (-inf, 1, 1),
           "y+inf": (1, inf, 1), "y-inf": (1, -inf, 1), "z+inf": (1, 1, inf), "z-inf": (1, 1, -inf), "inf/inf": (inf, 1, inf), "level": (5, 0, 0)}
    p = np.array(list(pts.values()), F32)
    ang = ur.angle(p[:, 0], p[:, 1], p[:, 2])
    got = dict(zip(pts, ang))
    assert all(np.isnan(got[k]) for k in ("origin", "xnan", "ynan", "znan", "inf/inf"))
    assert all(got[k] == 0 for k in ("x+inf", "x-inf", "y+inf", "y-inf", "level")) and got["z+inf"] == 90 and got["z-inf"] == -90
    level = {16: 8, 32: 23, 64: 6}
    for n_scans in (16, 32, 64):
        rid, drop = ur.ring(ang, n_scans)
        res = dict(zip(pts, zip(rid.tolist(), drop.tolist())))
        for k in ("origin", "xnan", "ynan", "znan", "inf/inf"):
            assert res[k][1] and res[k][0] <= ur.INT_MIN + 32, "int(NaN) = INT_MIN: dropped in each table"
        for k in ("x+inf", "x-inf", "y+inf", "y-inf", "level"):
            assert res[k] == (level[n_scans], False)
        assert res["z+inf"][1] and res["z-inf"][1]
        assert ur.decided(p[:, 0], p[:, 1], p[:, 2], n_scans).all()
    for n_scans in (4, 128):
        rid, drop = ur.ring(ang, n_scans)
        assert not drop.any() and not rid.any()


# ---- the time column ----
def _to_f32(d):
    """the double d rounded to the nearest float32 (ties to even), exactly"""
    if d == 0:
        return 0.0
    _, e = math.frexp(d)
    ulp = Fraction(2) ** (e - 24)
    return float(round(Fraction(d) / ulp) * ulp)


@pytest.mark.parametrize("n_scans", ur.N_SCANS)
def test_time_column_against_exact_arithmetic(n_scans):
    period = float(Fraction(0.100859904) - Fraction(20.736e-6))
    assert period == ur.SCAN_PERIOD
    for i in (0, n_scans - 1, n_scans, 2 ** 20 + 3):
        a = float(Fraction(55.296e-6) * (i // n_scans))          # each double operation: the exact result, rounded once
        b = float(Fraction(2.304e-6) * (i % n_scans))
        rel = _to_f32(float(Fraction(float(Fraction(a) + Fraction(b))) / Fraction(period)))
        want = _to_f32(float(Fraction(rel) * Fraction(period)))
        got = ur.time_of(np.array([i]), n_scans)[0]
        assert got.dtype == F32 and float(got) == want, (i, float(got), want)
    assert ur.time_of(np.array([0]), n_scans)[0] == 0 and ur.time_of(np.array([n_scans]), n_scans)[0] == F32(55.296e-6)


# ---- the kernel's arithmetic header, compiled for the host ----
def test_host_build_of_the_arithmetic_header_gives_the_same_bits(tmp_path):
    src = tmp_path / "um.cpp"
    src.write_text('#include <cstdio>\n#include <cstring>\n#include "untimed_math.h"\nint main() {\n  float p[3]; unsigned i; int s;\n'
                   '  while (std::scanf("%a %a %a %u %d", &p[0], &p[1], &p[2], &i, &s) == 5) {\n'
                   '    const float a = soicp::untimed_angle(p[0], p[1], p[2]), t = soicp::untimed_time(i, (unsigned)s);\n'
                   '    unsigned ab, tb; std::memcpy(&ab, &a, 4); std::memcpy(&tb, &t, 4);\n'
                   '    std::printf("%u %d %u\\n", ab, soicp::untimed_ring(a, s), tb);\n  }\n  return 0;\n}\n')
    exe = tmp_path / "um"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "superodom_amd", "csrc"), str(src), "-o", str(exe)])
    for n_scans in ur.N_SCANS:
        v = ur.sweep(1500, n_scans, seed=40 + n_scans, drop_share=0.2)
        b = np.array(_boundaries(n_scans if n_scans in (16, 32, 64) else 16))
        bx, by, bz = _at_elevation(np.concatenate([b - 1e-3, b + 1e-3]))
        x, y, z = np.concatenate([v["x"], bx, [np.nan, np.inf, 1]]), np.concatenate([v["y"], by, [1, 1, 1]]), np.concatenate([v["z"], bz, [1, np.inf, -np.inf]])
        x, y, z = x.astype(F32), y.astype(F32), z.astype(F32)
        idx = np.arange(len(x)) * 701 + 5
        text = "".join(f"{float(a).hex()} {float(b_).hex()} {float(c).hex()} {i} {n_scans}\n" for a, b_, c, i in zip(x, y, z, idx))
        out = np.array(subprocess.check_output([str(exe)], input=text.encode()).split(), np.int64).reshape(-1, 3)
        ang = ur.angle(x, y, z)
        rid, drop = ur.ring(ang, n_scans)
        same_angle = (out[:, 0] == ang.view(np.uint32)) | np.isnan(ang)
        assert same_angle.all() and np.array_equal(out[:, 1] < 0, drop) and np.array_equal(out[~drop, 1], rid[~drop])
        assert np.array_equal(out[:, 2], ur.time_of(idx, n_scans).view(np.uint32))


# ---- the same header, compiled for the device with the build's flags ----
def test_device_build_of_the_angle_has_the_correctly_rounded_sqrt_and_quotient(tmp_path):
    """untimed_angle pins sqrt and the quotient as correctly rounded.  For gfx950 that is v_sqrt_f32 followed by the +-1 ulp fix-up
    (the two neighbours formed with integer adds, each tested with an fma residual) and the v_div_scale / v_div_fmas / v_div_fixup
    sequence; an intrinsic or a fast-math flag that leaves the bare 1 ulp v_sqrt_f32 or v_rcp_f32 behind fails here"""
    from superodom_amd import build as B
    src = tmp_path / "angle.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "untimed_math.h"\n'
                   '__global__ void angle_kernel(const float* p, float* o) { o[threadIdx.x] = soicp::untimed_angle(p[0], p[1], p[2]); }\n')
    asm = tmp_path / "angle.s"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), f"--offload-arch={B.ARCH}", "--cuda-device-only", "-S", "-I", B.CSRC,
                           str(src), "-o", str(asm)] + B.COMMON, stderr=subprocess.DEVNULL)
    text = asm.read_text()
    ops = [ln.split()[0] for ln in text[text.index("angle_kernel"):].splitlines() if ln.startswith("\t") and ln.split() and ln.split()[0][:2] in ("v_", "s_")]
    assert ops.count("v_sqrt_f32_e32") == 1
    after = ops[ops.index("v_sqrt_f32_e32"):ops.index("v_div_scale_f32")]  # the quotient needs the root: its code follows
    assert after.count("v_add_u32_e32") == 2 and after.count("v_fma_f32") == 2, after
    assert ops.count("v_div_scale_f32") == 2 and ops.count("v_div_fmas_f32") == 1 and ops.count("v_div_fixup_f32") == 1


# ---- the GPU tests' data ----
def _drop_pattern(v, n_scans):
    return ur.ring(ur.angle(v["x"], v["y"], v["z"]), n_scans)[1]


def test_gpu_sweeps_are_decided_and_carry_their_cases():
    """the condition on the inputs that lets test_gpu_untimed.py compare bit for bit: no point of any sweep sits where the last bit
    of the float atan, or the overload choice, decides its ring (sweep() asserts it and draws such a point again)"""
    for name, kw in ur.GPU_SWEEPS.items():
        v = ur.gpu_sweep(name)
        n, n_scans = kw["n"], kw["n_scans"]
        assert len(v["x"]) == n and ur.decided(v["x"], v["y"], v["z"], n_scans).all(), name
        drop = _drop_pattern(v, n_scans)
        k = ur.kept_by_prefix_rule(drop)
        if n_scans in (4, 128):
            assert not drop.any() and len(k) == n
            continue
        if name == "all_dropped":
            assert drop.all() and len(k) == 0
            continue
        if n >= ur.TILE:
            tiles = [drop[s:s + ur.TILE] for s in range(0, n, ur.TILE)]
            assert all(t.any() for t in tiles[:-1]) and drop.any(), (name, "drops in every full tile")
            assert 0 < len(k) < n - drop.sum(), (name, "the cut-off tail holds points that would have been kept")
    # the truncation cases by name
    v = ur.gpu_sweep(f"n{3 * ur.TILE + 17}")
    drop = _drop_pattern(v, 16)
    k = ur.kept_by_prefix_rule(drop)
    cut = k[-1] + 1                      # at or just in front of the first unvisited index
    assert cut < 3 * ur.TILE < len(drop), "the cut-off tail spans a tile boundary"
    assert drop[cut:].sum() >= 10 and (~drop[cut:]).sum() >= 10, "and contains would-be drops and would-be records"
    v = ur.gpu_sweep("long")
    k = ur.kept_by_prefix_rule(_drop_pattern(v, 16))
    assert len(v["x"]) == 66 * ur.TILE + 5 and k[-1] >= 65 * ur.TILE, "a workgroup with more than 64 in front of it stores records"
