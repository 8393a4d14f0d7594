"""CPU: what the batch's and the run's correspondence exports share and what can be held of it without a device -- the prefix table of
the entries' tile counts (reg_plan.h: selection_tile_table), ticket -> (entry, tile) over it (selection_ticket) with entries of no tile
first, in the middle and last, the table entry the kernels read (corr_kernels.h: CorrSelEntry, 104 bytes, scan_at behind the rest).
tests/native/selection_correspondences_host.cpp is also a program of its own (-DSELECTION_HOST_MAIN) that walks the same cases: the form
in which the layout functions are built with -fsanitize=address,undefined."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sequence_correspondences_data as scd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "selection_correspondences_host.cpp")
LIB = os.path.join(HERE, "native", "libselection_correspondences_host.so")
HDR = os.path.join(ROOT, "superodom_amd", "csrc")
U32P = C.POINTER(C.c_uint32)
TILE = scd.TILE

# points per entry of a selection, 0 for an entry without a set
CASES = {
    "all_equal": [4096] * 5,
    "zero_first": [0, 2049, 1025],
    "zero_middle": [2049, 0, 1025],
    "zero_last": [2049, 1025, 0],
    "all_zero": [0, 0, 0, 0],
    "one_point": [1],
    "one_tile": [TILE],
    "one_tile_and_a_point": [TILE + 1],
    "tile_edges": [1, TILE, TILE + 1, 0, TILE + 1, TILE, 1],
    "no_entry": [],
}


@pytest.fixture(scope="module")
def native():
    deps = [SRC] + [os.path.join(HDR, h) for h in ("reg_plan.h", "so_math.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-fPIC", "-shared", "-I", HDR, SRC, "-o", LIB])
    L = C.CDLL(LIB)
    L.sel_tile_table.argtypes = [U32P, C.c_uint32, C.c_uint32, U32P]; L.sel_tile_table.restype = C.c_uint32
    L.sel_ticket.argtypes = [C.c_uint32, U32P, C.c_uint32, U32P]; L.sel_ticket.restype = None
    return L


def _table(native, points):
    n = np.asarray(points, np.uint32)
    first = np.full(len(points) + 1, 0xDEADBEEF, np.uint32)
    tiles = native.sel_tile_table(n.ctypes.data_as(U32P), len(points), TILE, first.ctypes.data_as(U32P))
    return tiles, first


@pytest.mark.parametrize("case", list(CASES))
def test_the_prefix_table_of_tile_counts(native, case):
    points = CASES[case]
    tiles, first = _table(native, points)
    want = [(n + TILE - 1) // TILE for n in points]
    assert list(first) == [sum(want[:k]) for k in range(len(points) + 1)] and tiles == sum(want)
    assert np.array_equal(first, scd.tile_first(points)), "the table the GPU tests' data module states"
    if case == "all_equal":
        assert list(first) == [k * 4 for k in range(6)], "a batch: tile_first[k] = k * nblk"
    if case in ("all_zero", "no_entry"):
        assert tiles == 0 and not first.any(), "nothing to launch"


@pytest.mark.parametrize("case", list(CASES))
def test_every_ticket_is_worked_once_behind_its_predecessors(native, case):
    """every ticket 0 .. tile_first[n_sel] - 1 maps to an (entry, tile) that exists, each once, in entry-major order; the look-back chain
    of a tile -- the tiles below it in the same entry -- holds smaller tickets only; an entry without tiles gets no ticket"""
    points = CASES[case]
    tiles, first = _table(native, points)
    out = (C.c_uint32 * 2)()
    got = []
    for t in range(tiles):
        native.sel_ticket(t, first.ctypes.data_as(U32P), len(points), out)
        k, tile = out[0], out[1]
        assert (k, tile) == scd.ticket_ref(t, first)
        assert tile < (points[k] + TILE - 1) // TILE
        assert all(int(first[k]) + below < t for below in range(tile)), "a predecessor of the chain with a larger ticket"
        got.append((k, tile))
    assert got == [(k, b) for k in range(len(points)) for b in range((points[k] + TILE - 1) // TILE)]


def test_the_table_entry_the_kernels_read():
    """CorrSelEntry as the host fills it: the ctypes mirror of the declaration is 104 bytes with scan_at at 96 -- behind the 96 bytes the
    run's export always had --, and the header holds the build to the same two numbers"""
    text = open(os.path.join(HDR, "corr_kernels.h")).read()
    body = re.search(r"struct CorrSelEntry \{(.*?)\};", text, re.S).group(1)
    kinds = {"unsigned long long": C.c_uint64, "double": C.c_double, "uint32_t": C.c_uint32, "int32_t": C.c_int32}
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        kind, names = re.match(r"(unsigned long long|double|uint32_t|int32_t)\s+(.*)", decl).groups()
        for name in [n.strip() for n in names.split(",")]:
            m = re.match(r"(\w+)\[(\d+)\]", name)
            fields.append((m.group(1), kinds[kind] * int(m.group(2))) if m else (name, kinds[kind]))
    Entry = type("Entry", (C.Structure,), {"_fields_": fields})
    assert [f[0] for f in fields] == ["at", "rec_first", "status_first", "a2", "pose", "n", "variant", "scan_at"]
    assert C.sizeof(Entry) == 104 and Entry.scan_at.offset == 96 and Entry.pose.offset == 32 and Entry.n.offset == 88
    assert "static_assert(sizeof(CorrSelEntry) == 104 && offsetof(CorrSelEntry, scan_at) == 96" in text

