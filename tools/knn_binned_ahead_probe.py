#!/usr/bin/env python3
"""Probe of an OPEN exactness question of the chunked sweep (profiles/knn_second_pass/README.md, section 5; present before that change):
python tools/knn_binned_ahead_probe.py

The queries of tests/knn_second_pass_data.bounded() behind 64 of them taken from two cubes, announced (so_icp_stage_scan), binned ahead
by a registration 100 m away and then registered under the identity, 12 times per variant (`dup`: the 64 also stay in the scan; `nodup`:
they do not) on the instrumented and the production instantiation.  Logs, per registration, whether it was binned ahead and every
neighbour list that differs from the numpy brute force.  Seen so far: in a few registrations in a hundred, always binned ahead, the easy
query (-19.600079, -19.598434, -19.60348) -- 5th and 6th neighbour 6e-6 apart in d2 -- gets the 6th in place of the 5th."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
os.environ.setdefault("SOICP_CACHE", os.path.join(ROOT, ".soicp_cache"))
import knn_edge_data as ked
import knn_second_pass_data as spd
from superodom_amd import binding as soicp
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
fam = spd.bounded()
def product(**kw):
    s = soicp.LidarSlamGpu(plane_res=fam.plane_res, line_res=fam.plane_res / 2, max_surface_features=-1, max_iterations=1, **kw)
    s.add_surf_point_cloud(fam.map_points)
    return s
s0 = product(); exp = s0.export_map(); s0.close()
q = fam.queries
filler = np.array([[3.0, 40.0, 9.0]], np.float32) + np.arange(4200 - len(q), dtype=np.float32)[:, None] * np.array([[0.001, 0, 0]], np.float32)
scan = np.ascontiguousarray(np.concatenate([q, filler]), np.float32)
sa = next(s for s in fam.info["sites"] if s["name"] == "a/ordinary")
sf = [s for s in fam.info["sites"] if s["kind"] == "f"]
ia = np.arange(sa["first_query"], sa["first_query"] + 32)
i_f = np.concatenate([np.arange(s["first_query"], s["first_query"] + s["n_queries"]) for s in sf])[:32]
head = np.empty((64, 3), np.float32); head[0::2], head[1::2] = q[ia], q[i_f]
rest = np.delete(scan, np.concatenate([ia, i_f]), axis=0)
for name, B_np in (("dup", np.concatenate([head, scan])), ("nodup", np.concatenate([head, rest]))):
    B_np = np.ascontiguousarray(B_np, np.float32)
    rf, ridx, rd2, rnbr = ked.brute_knn(exp, B_np)
    gate = np.float64(np.float32(3) * np.float32(fam.plane_res))
    want = rf & (rd2[:, 4].astype(np.float64) <= gate)
    for mode in ("prof", "prod"):
        if mode == "prof":
            os.environ["SOICP_ABLATE"] = "65536"
        slam = product(**({"time_kernels": 2} if mode == "prof" else {}))
        os.environ.pop("SOICP_ABLATE", None)
        A, B = slam.host_alloc_like(fam.info["scan_a"]), slam.host_alloc_like(B_np)
        for attempt in range(12):
            slam.stage_scan(B)
            rc, _, _ = slam.register(A, fam.info["pose_a"])
            rc2, pose, st = slam.register(B, IDENT)
            ms, nb = slam.match_status(len(B_np)), slam.neighbours(len(B_np))
            judged = np.isin(ms, (0, 3, 4, 5))
            ahead = bool(st.flags & soicp.FLAG_BINNED_AHEAD)
            bad_status = int((judged != want).sum())
            both = judged & want
            # canonical index -> coordinates through the export (slot of the cube << 20 | position): compare coordinates of cube-local rows
            ec = ked.cube_of(exp); starts = {tuple(ec[i]): i for i in range(len(exp) - 1, -1, -1)}
            bad = []
            for i in np.nonzero(both)[0]:
                off = starts[tuple(ked.cube_of(rnbr[i, 0]))]
                got = exp[off + (nb[i].astype(np.int64) & ((1 << 20) - 1))]
                if not np.array_equal(got.view(np.uint32), rnbr[i].view(np.uint32)):
                    bad.append((int(i), got.tolist(), rnbr[i].tolist()))
            print(f"{name} {mode} attempt {attempt}: rc {rc} {rc2} ahead {ahead} status mismatches {bad_status} list mismatches {len(bad)}", flush=True)
            for b in bad[:3]:
                print("   B index", b[0], "query", B_np[b[0]].tolist(), "\n   got ", b[1], "\n   want", b[2], flush=True)
        slam.close()
