"""Numpy-only restatement of the DTU evaluation of the reference (evaluations/dtu: reducePts_haa.m, MaxDistCP.m,
PointCompareMain.m, BaseEvalMain_web.m / ComputeStat_web.m), used by the tests as the oracle of cds_mvsnet_amd.dtu_eval.

Distances are fp32 (d2 = dx*dx + dy*dy + dz*dz, then sqrt) like the GPU path; masks and statistics are float64 like MATLAB."""
import numpy as np


def d2_f32(a, b):
    """fp32 squared distances [len(a), len(b)] in the order dx*dx + dy*dy + dz*dz."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    dx = b[None, :, 0] - a[:, None, 0]
    dy = b[None, :, 1] - a[:, None, 1]
    dz = b[None, :, 2] - a[:, None, 2]
    return dx * dx + dy * dy + dz * dz


def reduce_pts(pts, dst, order):
    """reducePts_haa.m: visit the points in ``order``; a point still kept removes every point within dst (d2 <= dst^2,
    fp32) and stays itself.  -> bool keep mask."""
    pts = np.asarray(pts, np.float32)
    dst2 = np.float32(dst) * np.float32(dst)
    keep = np.ones(len(pts), bool)
    for i in np.asarray(order):
        if keep[i]:
            keep[(d2_f32(pts[i:i + 1], pts)[0] <= dst2)] = False
            keep[i] = True
    return keep


def brute_nn(q, t):
    """fp32 brute-force nearest-neighbour distance of every q in t (inf for an empty t)."""
    q = np.asarray(q, np.float32)
    out = np.full(len(q), np.inf, np.float32)
    if len(t) == 0:
        return out
    chunk = max(1, (1 << 21) // len(t))
    for s in range(0, len(q), chunk):
        out[s:s + chunk] = np.sqrt(d2_f32(q[s:s + chunk], t).min(1))
    return out


def max_dist_cp(qto, qfrom, bb, max_dist):
    """MaxDistCP.m: blocks of side max_dist tile [BB(1,:), BB(1,:) + (floor((BB(2,:) - BB(1,:)) / max_dist) + 1) max_dist);
    the from-points of a block search the to-points of the block grown by max_dist on each side (brute force here);
    every other from-point gets max_dist."""
    qto = np.asarray(qto, np.float32)
    qfrom = np.asarray(qfrom, np.float32)
    bb = np.asarray(bb, np.float64)
    dist = np.full(len(qfrom), max_dist, np.float64)
    rng = np.floor((bb[1] - bb[0]) / max_dist).astype(int)
    f64, t64 = qfrom.astype(np.float64), qto.astype(np.float64)
    for x in range(rng[0] + 1):
        for y in range(rng[1] + 1):
            for z in range(rng[2] + 1):
                low = bb[0] + np.array([x, y, z]) * max_dist
                high = low + max_dist
                idx_f = np.nonzero(((f64 >= low) & (f64 < high)).all(1))[0]
                if len(idx_f) == 0:
                    continue
                idx_t = np.nonzero(((t64 >= low - max_dist) & (t64 < high + max_dist)).all(1))[0]
                if len(idx_t) == 0:
                    dist[idx_f] = max_dist
                else:
                    dist[idx_f] = brute_nn(qfrom[idx_f], qto[idx_t])
    return dist


def block_grid_member(qfrom, bb, max_dist):
    """The from-points that MaxDistCP.m's block loop visits (the others keep max_dist)."""
    q = np.asarray(qfrom, np.float32).astype(np.float64)
    bb = np.asarray(bb, np.float64)
    seen = np.zeros(len(q), bool)
    rng = np.floor((bb[1] - bb[0]) / max_dist).astype(int)
    for x in range(rng[0] + 1):
        for y in range(rng[1] + 1):
            for z in range(rng[2] + 1):
                low = bb[0] + np.array([x, y, z]) * max_dist
                seen |= ((q >= low) & (q < low + max_dist)).all(1)
    return seen


def matlab_round(x):
    t = np.trunc(x)
    return t + np.sign(x) * (np.abs(x - t) >= 0.5)


def data_in_mask(q, obs, bb, res):
    """PointCompareMain.m:30-41 (float64, 1-based, column-major sub2ind)."""
    qv = matlab_round((np.asarray(q, np.float64) - np.asarray(bb, np.float64)[0]) / res + 1.0)
    size = np.array(obs.shape)
    inside = ((qv > 0) & (qv <= size)).all(1)
    out = np.zeros(len(q), bool)
    sub = qv[inside].astype(np.int64) - 1
    lin = np.ravel_multi_index((sub[:, 0], sub[:, 1], sub[:, 2]), obs.shape, order="F")
    out[np.nonzero(inside)[0]] = np.asarray(obs).ravel(order="F")[lin]
    return out


def above_plane(q, p):
    """PointCompareMain.m:53: P' * [q; 1] > 0 in float64."""
    q = np.asarray(q, np.float64)
    p = np.asarray(p, np.float64).reshape(4)
    return (q @ p[:3] + p[3]) > 0


def stats(d, max_dist):
    """BaseEvalMain_web.m:63-72 / ComputeStat_web.m:52-68: d < max_dist, then mean, median, var (n - 1), n."""
    d = np.asarray(d, np.float64)
    d = d[d < max_dist]
    if len(d) == 0:
        return {"mean": np.nan, "median": np.nan, "var": np.nan, "n": 0}
    return {"mean": float(d.mean()), "median": float(np.median(d)), "var": float(d.var(ddof=1)) if len(d) > 1 else 0.0,
            "n": int(len(d))}


def point_compare(qdata, gt, dst, order, max_dist=20.0, block=60.0):
    """PointCompareMain.m + the statistics of BaseEvalMain_web.m for one scan; ``block``: the MaxDistCP search cap
    (60 mm in the protocol).  -> dict with the per-point arrays and the statistics."""
    keep = reduce_pts(qdata, dst, order)
    data = np.asarray(qdata, np.float32)[keep]
    stl = np.asarray(gt["stl"], np.float32)
    ddata = max_dist_cp(stl, data, gt["BB"], block)
    dstl = max_dist_cp(data, stl, gt["BB"], block)
    in_mask = data_in_mask(data, gt["ObsMask"], gt["BB"], gt["Res"])
    above = above_plane(stl, gt["P"])
    acc, comp = stats(ddata[in_mask], max_dist), stats(dstl[above], max_dist)
    return {"keep": keep, "data": data, "ddata": ddata, "dstl": dstl, "data_in_mask": in_mask, "stl_above_plane": above,
            "acc": acc, "comp": comp, "overall": (acc["mean"] + comp["mean"]) / 2.0}
