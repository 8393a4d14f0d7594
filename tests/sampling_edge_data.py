"""Path-directed inputs for the first stage of a registration: the sampling rule (calculateSamplingRate / shouldProcessPoint,
LidarSlam.cpp:346-359) and the two ways its kept points reach the k-NN sweep -- binned into chunks, or dealt out one wavefront per
share (knn_query_wave_kernel).  Plain numpy: the table of (n, max_surface_features) pairs, a float64 restatement of the rule and of
the share partition (query_wave_first, launch_knn_query_waves: kernels.hip), the census of a pair's shares, and one scan builder.
test_sampling_edges_host.py asserts every number of the table on the CPU; test_gpu_sampling_edges.py runs the pairs."""
import numpy as np

QUERY_WAVE_MAX_KEPT = 4096  # kQueryWaveMaxKept (kernels.h)
DROPPED = 254               # SO_MATCH_DROPPED (kernels.hip)


# ------------------------------------------------------------------------------------------------------------------------
# the rule and the share partition, restated
# ------------------------------------------------------------------------------------------------------------------------
def keeps(n, msf):
    """bool [n]: the points the rule keeps of a scan of n points (sampling_keeps, kernels.hip; orc_should_process, so_oracle.c)"""
    if msf < 0 or n <= msf:
        return np.ones(n, bool)
    rate = np.float64(1.0) * np.float64(msf) / np.float64(n)
    rem = np.fmod(np.arange(n, dtype=np.float64) * rate, 1.0)
    return ~(rem + 0.001 > rate)


def kept_upper_bound(n, msf):
    """reg_plan.h"""
    return msf + 2 if (msf >= 0 and n > msf) else n


def takes_query_waves(n, msf):
    """query_wave_count_ok (reg_plan.h) with kQueryWaveMaxKept"""
    return n != 0 and kept_upper_bound(n, msf) <= QUERY_WAVE_MAX_KEPT


def wave_plan(n, msf):
    """(per_wave, n_waves) as launch_knn_query_waves derives them"""
    sampled = msf > 0 and n > msf
    return (np.float64(n) / np.float64(msf), msf + 1) if sampled else (np.float64(1.0), n)


def wave_first(k, n, per_wave):
    """query_wave_first for an array of wavefront numbers k"""
    k = np.asarray(k, dtype=np.int64)
    if per_wave <= 1.0:
        return np.minimum(k, n)
    f = np.ceil(k.astype(np.float64) * per_wave)
    return np.where(f < np.float64(n), f, np.float64(n)).astype(np.int64)


def shares(n, msf):
    """int64 [n_waves + 1]: share k of the scan is [bounds[k], bounds[k + 1]) -- i_lo and i_hi of wavefront k"""
    per_wave, n_waves = wave_plan(n, msf)
    return wave_first(np.arange(n_waves + 1), n, per_wave)


def census(n, msf):
    """What the shares of a pair look like: the kept points with their share and their offset inside it, and the counts the table states."""
    keep = keeps(n, msf)
    b = shares(n, msf)
    kept_idx = np.nonzero(keep)[0]
    share = np.searchsorted(b, kept_idx, side="right") - 1
    offset = kept_idx - b[share]
    per_share = np.bincount(share, minlength=len(b) - 1)
    length = np.diff(b)
    return dict(kept=int(keep.sum()), kept_idx=kept_idx, share=share, offset=offset, n_waves=len(b) - 1,
                empty=int((per_share == 0).sum()), two=int((per_share == 2).sum()), most=int(per_share.max(initial=0)),
                longest=int(length.max(initial=0)), trips=int((length.max(initial=0) + 63) // 64),
                late=kept_idx[offset >= 64], late_offsets=offset[offset >= 64])


# ------------------------------------------------------------------------------------------------------------------------
# the table: (n, msf) -> what the pair is for and what the host test must find.  kept: points the rule keeps.  `sampled` pairs
# (0 < msf < n) also state the census of their shares where the pair is named for it: late = kept points at offset >= 64 of their
# share (second trip of the share loop or later), late_at = the one offset all of them sit at, empty / two = shares without / with
# two kept points, longest = points of the longest share, trips = trips of the share loop for that share.
# ------------------------------------------------------------------------------------------------------------------------
PAIRS = {
    (13734, 210): dict(aim="kept points in the second trip", kept=210, late=25, late_at=65, empty=26, two=25, longest=66, trips=2),
    (27048, 210): dict(aim="kept points in the third trip", kept=210, late=25, late_at=128, empty=26, two=25, longest=129, trips=3),
    (6400, 100): dict(aim="shares of exactly 64 points", kept=100, late=0, longest=64, trips=1),
    (6500, 100): dict(aim="shares of exactly 65 points", kept=100, late=0, longest=65, trips=2),
    (6401, 100): dict(aim="shares that come out empty", kept=94, late=0, empty=7),
    (1000, 1): dict(aim="rate on 0.001, one wavefront, 16 trips", kept=1, late=0, trips=16),
    (1001, 1): dict(aim="rate under 0.001", kept=0, late=0, trips=16),
    (100000, 100): dict(aim="rate on 0.001 at 101 wavefronts", kept=100, late=0, trips=16),
    (100100, 100): dict(aim="rate under 0.001 at 101 wavefronts", kept=0, late=0, longest=1001, trips=16),
    (50000, 51): dict(aim="almost nothing kept", kept=1),
    (2, 1): dict(aim="smallest scans", kept=1),
    (3, 1): dict(aim="smallest scans", kept=1),
    (7, 3): dict(aim="smallest scans", kept=3),
    (4095, 4094): dict(aim="rate close to 1, shares of 1 to 3", kept=4090, empty=5),
    (8191, 4094): dict(aim="rate close to 1/2, shares of 1 to 3", kept=4086, empty=9),
    (12282, 4094): dict(aim="integer per_wave", kept=4094, empty=1, two=0),
    (5000, 4094): dict(aim="the switch: bound 4096 takes query waves", kept=4090),
    (5000, 4095): dict(aim="the switch: bound 4097 takes the chunked sweep", kept=4095),
    (4096, 4096): dict(aim="n == msf: no sampling", kept=4096),
    (4097, 4096): dict(aim="one point more than msf", kept=4092),
    (4097, 0): dict(aim="msf == 0: everything dropped, n_waves = n", kept=0),
    (100000, 0): dict(aim="msf == 0: everything dropped, n_waves = n", kept=0),
}
LATE_PAIRS = ((13734, 210), (27048, 210))
BIG_PAIRS = ((100000, 100), (100100, 100))  # run on the single-context front ends only


def pair_id(p):
    return f"{p[0]}-{p[1]}"


# ------------------------------------------------------------------------------------------------------------------------
# the scan
# ------------------------------------------------------------------------------------------------------------------------
def scan_of(scene, n, seed, index=0):
    """n points that all belong to the true pose scene.gt_pose(index): scene.scan(index) tiled to length n, the copies beyond the
    first with a seeded jitter of a few millimetres (no two queries alike)."""
    base = scene.scan(index)
    reps = -(-n // len(base))
    pts = np.tile(base, (reps, 1))[:n].astype(np.float64)
    rng = np.random.default_rng(seed)
    jitter = rng.uniform(-0.004, 0.004, pts.shape)
    jitter[:len(base)] = 0.0
    return np.ascontiguousarray((pts + jitter).astype(np.float32))
