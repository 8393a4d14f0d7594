"""The decisions of a registration's host schedule that need no device (superodom_amd/csrc/reg_plan.h: loop limits, the query split,
the query-wave switch, table and work-list sizes, the window rule of a chained start, which entry a pending pose prior refuses) compiled for the HOST and checked on the CPU.
so_icp_register, so_icp_register_sequence and so_icp_register_batch all take these from that one header."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "reg_plan_host.cpp")
LIB = os.path.join(HERE, "native", "libreg_plan_host.so")
HDR = os.path.join(ROOT, "superodom_amd", "csrc")
U64 = C.c_ulonglong


@pytest.fixture(scope="module")
def rp():
    deps = [SRC, os.path.join(HDR, "reg_plan.h"), os.path.join(HDR, "so_math.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-I", HDR, SRC, "-o", LIB])
    L = C.CDLL(LIB)
    i3, d3 = C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.rp_max_scan_points.restype = U64
    L.rp_kept_upper_bound.argtypes = [C.c_int, U64]; L.rp_kept_upper_bound.restype = U64
    L.rp_query_wave_count_ok.argtypes = [C.c_int, U64, U64]
    L.rp_query_split_share.argtypes = [U64, U64, U64, C.POINTER(U64)]; L.rp_query_split_share.restype = None
    L.rp_bin_table_log2.argtypes = [U64]; L.rp_bin_table_log2.restype = C.c_uint
    L.rp_work_list_fits.argtypes = [U64, U64]
    L.rp_cube_stable.argtypes = [i3, i3, d3, C.c_double]
    return L


def test_header_needs_no_device_headers():
    text = open(os.path.join(HDR, "reg_plan.h")).read()
    assert sorted(re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)) == ["algorithm", "cstddef", "cstdint", "so_math.h"]


def test_query_split_share(rp):
    out = (U64 * 3)()
    for world in range(1, 9):
        for n in range(0, 2 * 64 * world + 65 + 1):
            s_full, tail = divmod(n, 64)
            total = 0; tail_owners = []
            for rank in range(world):
                rp.rp_query_split_share(n, world, rank, out)
                own_full, own_tail, n_own = out[0], out[1], out[2]
                assert own_full == sum(1 for s in range(s_full) if s % world == rank), (n, world, rank)
                assert n_own == own_full * 64 + (tail if own_tail else 0), (n, world, rank)
                total += n_own
                if own_tail:
                    tail_owners.append(rank)
            assert total == n, (n, world)
            assert tail_owners == ([s_full % world] if tail else []), (n, world, tail_owners)


@pytest.mark.parametrize("n", [0, 1, 32768, 32769, 2 ** 20, 2 ** 21 - 1])
def test_bin_table_log2(rp, n):
    lg = rp.rp_bin_table_log2(n)
    assert lg >= 16
    assert 2 ** lg >= 2 * n
    assert lg == 16 or 2 ** (lg - 1) < 2 * n


def test_kept_upper_bound_and_the_query_wave_switch(rp):
    limit = 4096  # kQueryWaveMaxKept (kernels.h)
    assert rp.rp_query_wave_count_ok(-1, 4096, limit) and not rp.rp_query_wave_count_ok(-1, 4097, limit)
    assert rp.rp_query_wave_count_ok(4094, 100000, limit) and not rp.rp_query_wave_count_ok(4095, 100000, limit)
    assert rp.rp_kept_upper_bound(2000, 1500) == 1500
    assert rp.rp_kept_upper_bound(-1, 4096) == 4096 and rp.rp_kept_upper_bound(4094, 100000) == 4096 and rp.rp_kept_upper_bound(4095, 100000) == 4097
    assert not rp.rp_query_wave_count_ok(-1, 0, limit)  # (an empty scan is not swept at all)


def test_limits(rp):
    from superodom_amd import binding
    assert rp.rp_outer_cap() == binding.MAX_OUTER == 16
    for v in (0, -1, -1000):
        assert rp.rp_outer_limit(v) == 4 and rp.rp_lm_limit(v) == 4
    assert [rp.rp_outer_limit(v) for v in (1, 5, 16, 17, 1000)] == [1, 5, 16, 16, 16]
    assert [rp.rp_lm_limit(v) for v in (1, 4, 16, 17, 1000)] == [1, 4, 16, 16, 16]
    assert rp.rp_max_scan_points() == 2 ** 21


def test_work_list_fits(rp):
    limit = 1024 * 4  # kKnnBlocks wavefront quartets (kernels.h)
    kept = 0x1FFFFF    # (the low field is not part of the sum)
    for normal, light in ((limit, 0), (0, limit), (limit - 7, 7), (1, limit - 1)):
        assert rp.rp_work_list_fits(kept | normal << 21 | light << 42, limit), (normal, light)
        assert not rp.rp_work_list_fits(kept | (normal + 1) << 21 | light << 42, limit), (normal, light)
        assert not rp.rp_work_list_fits(kept | normal << 21 | (light + 1) << 42, limit), (normal, light)


def test_which_entry_is_refused_by_which_pending_prior(rp):
    kinds = (C.c_int * 4)()
    rp.rp_prior_kinds(kinds)
    none, single, run, batch = kinds
    assert len({none, single, run, batch}) == 4
    # rows: what the entry takes -- none: so_icp_match(_dev); single: so_icp_register(_dev), so_icp_localization(_dev), so_icp_set_pose_prior;
    # run: so_icp_register_sequence, so_icp_localization_sequence, so_icp_set_sequence_priors; batch: so_icp_register_batch,
    # so_icp_set_batch_priors.  Columns: what is pending.  The answer: nothing (go on), or the pending kind the refusal names
    table = {
        (none, none): none, (none, single): single, (none, run): run, (none, batch): batch,
        (single, none): none, (single, single): none, (single, run): run, (single, batch): batch,
        (run, none): none, (run, single): single, (run, run): none, (run, batch): batch,
        (batch, none): none, (batch, single): single, (batch, run): run, (batch, batch): none,
    }
    assert len(table) == 16
    for (accepted, pending), want in table.items():
        assert rp.rp_refused_prior(pending, accepted) == want, (accepted, pending)


def test_carries_pose_prior(rp):
    # a pending single prior goes into the context's own registration on one device; so_icp_match never carries one
    assert rp.rp_carries_pose_prior(1, 1, 1, 0) and rp.rp_carries_pose_prior(1, 1, 0, 0)
    for args in ((0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 2, 0), (1, 1, 1, 1)):
        assert not rp.rp_carries_pose_prior(*args), args


def test_cube_stable(rp):
    dims = (21, 21, 11)     # kMapW, kMapH, kMapD (local_map.h)
    origin = (10, 10, 5)    # block index of coordinate c: floor((c + 25) / 50) + origin -- the centre block for a pose at 0
    margin = 1.0

    def stable(t):
        return bool(rp.rp_cube_stable((C.c_int * 3)(*origin), (C.c_int * 3)(*dims), (C.c_double * 3)(*t), margin))

    assert stable((0.0, 0.0, 0.0))
    assert stable((3.0, -7.0, 12.0))
    for a in range(3):
        def at(v):
            t = [0.0, 0.0, 0.0]; t[a] = v
            return t
        # block faces lie at -25 + 50 j: a pose `margin` below one reaches it, a little further away it does not; the same from above
        assert not stable(at(25.0 - margin)) and stable(at(25.0 - margin - 0.125))
        assert not stable(at(-25.0 + margin - 0.125)) and stable(at(-25.0 + margin))
        # block index 2 / dim - 3: the window would roll; 3 / dim - 4: it stays
        assert not stable(at(50.0 * (2 - origin[a]))) and stable(at(50.0 * (3 - origin[a])))
        assert not stable(at(50.0 * (dims[a] - 3 - origin[a]))) and stable(at(50.0 * (dims[a] - 4 - origin[a])))
