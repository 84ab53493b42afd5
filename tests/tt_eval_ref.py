"""Numpy float64 restatement of the Tanks and Temples F-score rules of DESIGN.md 1.6, used by the tests as the oracle of
cds_mvsnet_amd.tt_eval.  Neither the public toolbox nor Open3D is consulted: these rules are the specification.

Distances are fp32 (d2 = dx*dx + dy*dy + dz*dz, first minimum wins) like the GPU path; the transform is the explicit elementwise
float64 expression rounded once to fp32; voxel means, the crop, the pair sums, Umeyama and the scores are float64."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

N_SUMS = 18


def transform(points, T):
    """fp32(T p): row r = ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3] in float64, elementwise (no BLAS), rounded once."""
    p = np.asarray(points, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1).astype(np.float32)


def nearest_index(q, t, cap):
    """Brute force: fp32 d2, the first minimum (lowest index among equal d2), accepted iff d2 < cap*cap (fp32).
    -> (dist fp32: min(sqrt(d2), cap) or cap, index int32 or -1).

    Only to bound the work, the queries are visited in order of their coordinate along the target's longest axis, and a
    block of queries meets the targets within cap of the block along that axis, in ascending index order.  A target left
    out has |dx| > cap and so d2 >= cap*cap: it could not have been accepted, so the result is that of the full search."""
    q = np.asarray(q, np.float32)
    t = np.asarray(t, np.float32)
    cap = np.float32(cap)
    cap2 = cap * cap
    dist = np.full(len(q), cap, np.float32)
    index = np.full(len(q), -1, np.int32)
    if len(t) == 0 or len(q) == 0:
        return dist, index
    ax = int(np.argmax(t.max(0).astype(np.float64) - t.min(0)))
    t_by = np.argsort(t[:, ax], kind="stable")
    tx = t[t_by, ax].astype(np.float64)
    q_by = np.argsort(q[:, ax], kind="stable")
    reach = float(cap) * (1.0 + 1e-5) + 1e-30

    def block(s):
        rows = q_by[s:s + 256]
        a = q[rows]
        lo = np.searchsorted(tx, float(a[0, ax]) - reach, "left")
        hi = np.searchsorted(tx, float(a[-1, ax]) + reach, "right")
        if hi <= lo:
            return
        cand = np.sort(t_by[lo:hi])
        c = t[cand]
        dx = c[None, :, 0] - a[:, None, 0]
        dy = c[None, :, 1] - a[:, None, 1]
        dz = c[None, :, 2] - a[:, None, 2]
        d2 = dx * dx + dy * dy + dz * dz
        j = np.argmin(d2, 1)                                  # the first of equal minima = the lowest target index
        m = d2[np.arange(len(a)), j]
        hit = m < cap2
        index[rows] = np.where(hit, cand[j], -1)
        dist[rows] = np.where(hit, np.minimum(np.sqrt(m), cap), cap)

    with ThreadPoolExecutor(8) as pool:                       # blocks write disjoint rows; numpy releases the GIL
        list(pool.map(block, range(0, len(q), 256)))
    return dist, index


def pair_terms(p, q):
    """The [n, 18] float64 terms of the pair sums for fp32 pairs (p transformed source, q its target): 1, p, q, q p^T
    (row-major, q row), |p - q|^2 = (dx dx + dy dy) + dz dz, |p|^2."""
    p = np.asarray(p, np.float32).astype(np.float64).reshape(-1, 3)
    q = np.asarray(q, np.float32).astype(np.float64).reshape(-1, 3)
    d = p - q
    cols = [np.ones(len(p))] + [p[:, r] for r in range(3)] + [q[:, r] for r in range(3)]
    cols += [q[:, r] * p[:, c] for r in range(3) for c in range(3)]
    cols.append((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    cols.append((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    return np.stack(cols, 1)


def sum_terms(terms, reverse=False):
    """Sequential float64 sums of the columns, first pair to last (or last to first)."""
    if len(terms) == 0:
        return np.zeros(N_SUMS)
    return np.cumsum(terms[::-1] if reverse else terms, 0)[-1]


def pair_sums(source, T, target, cap, reverse=False):
    """One registration step: p = fp32(T source), q = nearest target of p; the 18 sums over the accepted pairs."""
    p = transform(source, T)
    _, idx = nearest_index(p, target, cap)
    hit = idx >= 0
    return sum_terms(pair_terms(p[hit], np.asarray(target, np.float32)[idx[hit]]), reverse)


# ------------------------------------------------------------------------------------------------------------- voxels
def voxel_keys(points, voxel):
    """Origin o = float32(min - voxel / 2); voxel index floorf((p - o) / v) per axis in fp32; the 63-bit key puts the
    index >> 3 of x, y, z (18 bits each) above the low three bits of x, y, z: ascending key = the output order."""
    p = np.asarray(points, np.float32)
    v = np.float32(voxel)
    o = (p.min(0).astype(np.float64) - 0.5 * float(voxel)).astype(np.float32)
    c = np.floor((p - o[None, :]) / v).astype(np.int64)
    c = np.maximum(c, 0)
    coarse = ((c[:, 0] >> 3) << 36) | ((c[:, 1] >> 3) << 18) | (c[:, 2] >> 3)
    local = ((c[:, 0] & 7) << 6) | ((c[:, 1] & 7) << 3) | (c[:, 2] & 7)
    return (coarse << 9) | local


def voxel_down_sample(points, voxel):
    """-> (means fp32 [V,3] in ascending key order, keys int64 [V], counts int64 [V]); each mean accumulated in float64 in
    input order, divided by the count, rounded once."""
    p = np.asarray(points, np.float32)
    if len(p) == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    keys = voxel_keys(p, voxel)
    order = np.argsort(keys, kind="stable")
    ukeys, first, counts = np.unique(keys[order], return_index=True, return_counts=True)
    sums = np.zeros((len(ukeys), 3))
    sp = p[order].astype(np.float64)
    for k in range(int(counts.max())):                      # k-th point of every voxel that has one: sequential per voxel
        sel = counts > k
        sums[sel] += sp[first[sel] + k]
    return (sums / counts[:, None]).astype(np.float32), ukeys.astype(np.int64), counts.astype(np.int64)


# --------------------------------------------------------------------------------------------------------------- crop
_UV = {"X": (1, 2, 0), "Y": (0, 2, 1), "Z": (0, 1, 2)}


def crop_mask(points, crop):
    """axis_min <= p[w] <= axis_max and an odd number of polygon edges (a, b) with (p[v] < a[v]) != (p[v] < b[v]) and
    a[u] + (p[v] - a[v]) / (b[v] - a[v]) * (b[u] - a[u]) < p[u], in float64."""
    p = np.asarray(points, np.float32).astype(np.float64)
    iu, iv, iw = _UV[crop["orthogonal_axis"]]
    poly = np.asarray(crop["bounding_polygon"], np.float64)
    u, v, w = p[:, iu], p[:, iv], p[:, iw]
    inside = np.zeros(len(p), bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(len(poly)):
            a, b = poly[i], poly[(i + 1) % len(poly)]
            straddles = (v < a[iv]) != (v < b[iv])
            x = a[iu] + (v - a[iv]) / (b[iv] - a[iv]) * (b[iu] - a[iu])
            inside ^= straddles & (x < u)
    return inside & (w >= crop["axis_min"]) & (w <= crop["axis_max"])


# ---------------------------------------------------------------------------------------------------------------- ICP
def umeyama(sums, with_scaling=True):
    """The similarity (or rigid) update that maps the p of the pair sums onto their q in the least-squares sense -> 4x4."""
    s = np.asarray(sums, np.float64)
    n = s[0]
    mp, mq = s[1:4] / n, s[4:7] / n
    cov = s[7:16].reshape(3, 3) / n - np.outer(mq, mp)
    var_p = s[17] / n - mp @ mp
    U, D, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    scale = float(np.trace(np.diag(D) @ S) / var_p) if with_scaling else 1.0
    out = np.eye(4)
    out[:3, :3] = scale * R
    out[:3, 3] = mq - scale * (R @ mp)
    return out


def _quality(s, m):
    return (s[0] / m, float(np.sqrt(s[16] / s[0])) if s[0] > 0 else 0.0)


def icp(source, target, cap, max_iter=20, rel_fitness=1e-6, rel_rmse=1e-6, with_scaling=True, init=None, reverse=False):
    """Point-to-point ICP -> (T, fitness, rmse, iterations); every evaluation re-transforms the original source."""
    T = np.eye(4) if init is None else np.asarray(init, np.float64).copy()
    m = len(source)
    if m == 0 or len(target) == 0:
        return T, 0.0, 0.0, 0
    s = pair_sums(source, T, target, cap, reverse)
    fit, rmse = _quality(s, m)
    it = 0
    while it < max_iter and s[0] >= 3:
        T = umeyama(s, with_scaling) @ T
        it += 1
        s = pair_sums(source, T, target, cap, reverse)
        nfit, nrmse = _quality(s, m)
        stop = abs(nfit - fit) < rel_fitness and abs(nrmse - rmse) < rel_rmse
        fit, rmse = nfit, nrmse
        if stop:
            break
    return T, fit, rmse, it


MAX_POINTS = 4_000_000


def every_kth(points):
    n = len(points)
    if n > MAX_POINTS:
        return points[::max(int(round(n / MAX_POINTS)), 1)]
    return points


def register(pred, gt, crop, init, tau, reverse=False):
    """Three ICP rounds, each from the previous transform -> (T, [iterations per round])."""
    T = np.asarray(init, np.float64).copy()
    pred = np.asarray(pred, np.float32)
    gt = np.asarray(gt, np.float32)
    t_crop = gt[crop_mask(gt, crop)]
    its = []
    for voxel, cap in ((tau, 80 * tau), (tau / 2, 20 * tau), (None, 2 * tau)):
        s = transform(pred, T)
        s = s[crop_mask(s, crop)]
        if voxel is None:
            s, t = every_kth(s), every_kth(t_crop)
        else:
            s, t = voxel_down_sample(s, voxel)[0], voxel_down_sample(t_crop, voxel)[0]
        R, _, _, it = icp(s, t, cap, init=None, reverse=reverse)
        T = R @ T
        its.append(it)
    return T, its


# -------------------------------------------------------------------------------------------------------------- score
def fscore(d1, d2, tau):
    """precision = #(d1 < tau) / len(d1), recall likewise on d2, F = 2PR / (P + R); 0 when a side is empty or P + R = 0."""
    if len(d1) == 0 or len(d2) == 0:
        return 0.0, 0.0, 0.0
    p = float((np.asarray(d1, np.float64) < tau).sum()) / len(d1)
    r = float((np.asarray(d2, np.float64) < tau).sum()) / len(d2)
    return p, r, (2 * p * r / (p + r) if p + r > 0 else 0.0)


def curve(d, tau, bins=500):
    """Cumulative share of the distances below (k + 1) tau / 100, k = 0 .. bins - 1."""
    edges = (np.arange(bins) + 1.0) * (tau / 100.0)
    d = np.sort(np.asarray(d, np.float64))
    return np.searchsorted(d, edges, side="left") / max(len(d), 1)


def evaluate(pred, gt, crop, trans, tau, do_register=True, reverse=False):
    pred = np.asarray(pred, np.float32)
    gt = np.asarray(gt, np.float32)
    T, its = register(pred, gt, crop, trans, tau, reverse) if do_register else (np.asarray(trans, np.float64), [])
    s = transform(pred, T)
    s_crop = s[crop_mask(s, crop)]
    t_crop = gt[crop_mask(gt, crop)]
    s_ds = voxel_down_sample(s_crop, tau / 2)[0]
    t_ds = voxel_down_sample(t_crop, tau / 2)[0]
    d1 = nearest_index(s_ds, t_ds, 5 * tau)[0]
    d2 = nearest_index(t_ds, s_ds, 5 * tau)[0]
    p, r, f = fscore(d1, d2, tau)
    return {"precision": p, "recall": r, "fscore": f, "transform": T, "iterations": its, "d1": d1, "d2": d2,
            "n_pred_cropped": len(s_crop), "n_gt_cropped": len(t_crop), "n_pred_sampled": len(s_ds), "n_gt_sampled": len(t_ds)}
