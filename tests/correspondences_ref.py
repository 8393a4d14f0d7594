"""Plain-numpy restatement of so_icp_correspondences (include/so_icp.h): what the export must give for the correspondences the oracle
formed (oracle_py CORR_DTYPE), a pose, plane_res and the Tukey variant.  The arithmetic is the evaluation's (kernels.hip eval_pass,
lidarOptimization.cpp:59-74), in numpy's own order of operations: agreement with the device is to a bound, not to the bit."""
import numpy as np

RECORD_DTYPE = np.dtype([("index", "<u4"), ("p", "<f4", 3), ("n", "<f8", 3), ("d", "<f8"), ("coeff", "<f8"), ("residual", "<f8"),
                         ("weight", "<f8")])
NOT_SAMPLED = 254  # the status byte of a point the sampling rule dropped (the oracle's -1)
EPS = 2.0 ** -53


def tukey_a2(plane_res):
    """TukeyLoss(a)'s a^2, a = (double)sqrtf(3 * planeRes) with the product in float (LidarSlam.cpp:271)"""
    a = np.float64(np.sqrt(np.float32(3) * np.float32(plane_res), dtype=np.float32))
    return a * a


def rotation(q):
    """Eigen::Quaternion::toRotationMatrix of (x, y, z, w)"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rotate(q, p):
    """Eigen::QuaternionBase::_transformVector: v + w * uv + u x uv with uv = 2 (u x v)"""
    u = np.asarray(q[:3], float)
    uv = 2.0 * np.cross(u, p)
    return p + q[3] * uv + np.cross(u, uv)


def loss(r, coeff, a2, variant):
    """(0.5 * coeff * rho(r^2), coeff * rho'(r^2)) of ScaledLoss(TukeyLoss(a), coeff): cost term and weight per residual"""
    s = r * r
    inside = s <= a2
    v = 1.0 - s / a2
    rho_out = a2 / 6.0 if variant == 0 else a2 / 3.0
    rho = np.where(inside, rho_out * (1.0 - v ** 3), rho_out)
    rho1 = np.where(inside, (0.5 if variant == 0 else 1.0) * v * v, 0.0)
    return 0.5 * coeff * rho, coeff * rho1


def residuals(p, n, d, pose):
    """n . (R(q) p + t) + d for float or double points p [N, 3]"""
    pose = np.asarray(pose, float)
    w = rotate(pose[3:], np.asarray(p, np.float64)) + pose[:3]
    return np.einsum("ij,ij->i", n, w) + d


def normal_equations(p, n, r, w, pose):
    """(JtJ [6, 6], Jtr [6], sum |JtJ terms| [6, 6], sum |Jtr terms| [6]) with J = [n, p x (R^T n)], JtJ += w J J^T, Jtr += w r J"""
    R = rotation(np.asarray(pose, float)[3:])
    J = np.concatenate([n, np.cross(np.asarray(p, np.float64), n @ R)], axis=1)  # (R^T n) as rows: n @ R
    terms = w[:, None, None] * J[:, :, None] * J[:, None, :]
    tr = (w * r)[:, None] * J
    return terms.sum(0), tr.sum(0), np.abs(terms).sum(0), np.abs(tr).sum(0)


def expected(corrs, pose, plane_res, variant=0):
    """What the export gives for oracle correspondences `corrs` (CORR_DTYPE, indexed like the scan) at `pose`:
    dict(records, status, residual, cost, cost_abs, JtJ, Jtr, JtJ_abs, Jtr_abs)."""
    st = corrs["status"]
    acc = np.flatnonzero(st == 0)
    a2 = tukey_a2(plane_res)
    rec = np.zeros(len(acc), RECORD_DTYPE)
    rec["index"] = acc
    rec["p"] = corrs["p"][acc].astype(np.float32)  # (the oracle holds the float scan point widened to double)
    rec["n"] = corrs["n"][acc]; rec["d"] = corrs["d"][acc]; rec["coeff"] = corrs["coeff"][acc]
    r = residuals(rec["p"], rec["n"], rec["d"], pose)
    term, w = loss(r, rec["coeff"], a2, variant)
    rec["residual"] = r; rec["weight"] = w
    status = np.where(st < 0, NOT_SAMPLED, st).astype(np.uint8)
    resid = np.full(len(corrs), np.nan, np.float32)
    resid[acc] = r.astype(np.float32)
    JtJ, Jtr, JtJ_abs, Jtr_abs = normal_equations(rec["p"], rec["n"], r, w, pose)
    return dict(records=rec, status=status, residual=resid, cost=float(term.sum()), cost_abs=float(np.abs(term).sum()), JtJ=JtJ, Jtr=Jtr,
                JtJ_abs=JtJ_abs, Jtr_abs=Jtr_abs, a2=a2)


def check_fields_at(rec, pose, a2, variant, tag):
    """residual and weight of every record (RECORD_DTYPE fields) against numpy from the record's own fields"""
    if not len(rec):
        return
    r = residuals(rec["p"], rec["n"], rec["d"], pose)
    _, w = loss(r, rec["coeff"], a2, variant)
    r_bound = 64 * EPS * (np.linalg.norm(rec["p"].astype(np.float64), axis=1) + np.linalg.norm(pose[:3]) + np.abs(rec["d"]) + 1.0)
    # (|dw/dr| <= 2 coeff |r| / a^2 is variant 0's; variant 1's slope is twice that, inside the 64 roundings budgeted per residual)
    w_bound = r_bound * 2 * rec["coeff"] * np.abs(r) / a2 + 8 * EPS * rec["coeff"]
    print(f"{tag}: max residual error / bound {np.max(np.abs(rec['residual'] - r) / r_bound):.3f}, max weight error / bound "
          f"{np.max(np.abs(rec['weight'] - w) / np.maximum(w_bound, 1e-300)):.3f}")
    assert np.all(np.abs(rec["residual"] - r) <= r_bound), tag
    assert np.all(np.abs(rec["weight"] - w) <= w_bound), tag


def sum_bound(n_terms, abs_sum):
    """two fp64 summations of N terms in different orders, plus a few dozen roundings per term"""
    return (2 * n_terms + 64) * EPS * abs_sum


def composite_scan(real, tile):
    """Real points with runs of far points (x >= 5 000 m: outside the 21 x 21 x 11 window, status 1) spliced in: a run of 2 * tile far
    points that starts at an index which is no multiple of the tile -- so at least one whole tile of the export has no accepted
    point --, and a run of 64 aligned to a wavefront.  Returns (scan float32 [N, 3], mask of the far points)."""
    real = np.asarray(real, np.float32)
    a = tile - 24                                  # the long run starts 24 points short of a tile boundary
    b = (-(a + 2 * tile)) % 64 + 15 * 64           # real points up to the next multiple of 64, and 15 wavefronts more
    c = 1000
    assert len(real) >= a + b + c and a % tile and (a + 2 * tile + b) % 64 == 0
    far = lambda k, x0: np.stack([x0 + 0.5 * np.arange(k), (np.arange(k) % 7) - 3.0, np.ones(k)], axis=1).astype(np.float32)
    parts = [real[:a], far(2 * tile, 5000.0), real[a:a + b], far(64, 7000.0), real[a + b:a + b + c]]
    mask = np.concatenate([np.full(len(p), k % 2 == 1) for k, p in enumerate(parts)])
    return np.ascontiguousarray(np.concatenate(parts)), mask
