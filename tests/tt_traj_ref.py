"""Numpy float64 restatement of the trajectory-alignment RANSAC of DESIGN.md 1.6 (cds_ransac_similarity_f64), the oracle of
tests/test_tt_traj_*.py: the counter-based sampler in Python integers, Umeyama with scaling through ``np.linalg.svd``, the
score over all correspondences and the total order of the winner.  Everything before the SVD (the sums in draw order, the
means, the covariance, the variance) and the score given T are written operation for operation as the kernel has them, so
the two differ by what the two SVDs differ in, and by nothing else."""
import numpy as np

MASK = (1 << 64) - 1
COLLINEAR_RATIO = 1e-9


def splitmix64(seed, c):
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample(seed, h, n, k):
    """The k distinct indices of hypothesis h in draw order (n >= k)."""
    picks = []
    for j in range(k):
        r = (splitmix64(seed, h * 8 + j) * (n - j)) >> 64
        for p in sorted(picks):
            if p <= r:
                r += 1
        picks.append(r)
    return picks


def samples(seed, H, n, k):
    """int64 [H,k]."""
    return np.array([sample(seed, h, n, k) for h in range(H)], np.int64).reshape(H, k)


def umeyama_pairs(p, q):
    """Umeyama with scaling on pairs p, q [H,k,3] (sums over k in the given order) -> (T [H,4,4], ok bool [H], ratio [H]):
    ``ok`` false where the hypothesis is rejected (T is then the identity), ``ratio`` the singular-value ratio d2 / d1."""
    H, k = p.shape[:2]
    sp, sq, sqp, spp = np.zeros((H, 3)), np.zeros((H, 3)), np.zeros((H, 3, 3)), np.zeros(H)
    for j in range(k):
        a, b = p[:, j], q[:, j]
        sp += a
        sq += b
        sqp += b[:, :, None] * a[:, None, :]
        spp += (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    n = float(k)
    mp, mq = sp / n, sq / n
    var_p = spp / n - ((mp[:, 0] * mp[:, 0] + mp[:, 1] * mp[:, 1]) + mp[:, 2] * mp[:, 2])
    cov = sqp / n - mq[:, :, None] * mp[:, None, :]
    sane = np.isfinite(cov).all((1, 2))
    U, D, Vt = np.linalg.svd(np.where(sane[:, None, None], cov, 0.0))
    E = np.ones((H, 3))
    E[np.linalg.det(U) * np.linalg.det(Vt) < 0, 2] = -1.0
    R = (U * E[:, None, :]) @ Vt
    with np.errstate(all="ignore"):
        scale = (D * E).sum(1) / var_p
        T = np.zeros((H, 4, 4))
        T[:, 3, 3] = 1.0
        T[:, :3, :3] = scale[:, None, None] * R
        T[:, :3, 3] = mq - scale[:, None] * (R @ mp[:, :, None])[:, :, 0]
        ratio = np.where(D[:, 0] > 0, D[:, 1] / np.where(D[:, 0] > 0, D[:, 0], 1.0), 0.0)
    ok = sane & (var_p != 0.0) & (D[:, 1] > COLLINEAR_RATIO * D[:, 0]) & np.isfinite(T).all((1, 2))
    T[~ok] = np.eye(4)
    return T, ok, ratio


def score(src, dst, T, threshold, chunk=4096):
    """-> (count int32 [H], err2 [H]) of transforms T [H,4,4]: d2 = |T src_i - dst_i|^2 with the row expression
    ((T0 x + T1 y) + T2 z) + T3, inlier iff d2 < threshold^2, err2 the sequential sum of the inlier d2 in index order."""
    thr2 = threshold * threshold
    x, y, z = (src[None, :, c] for c in range(3))
    count, err2 = np.zeros(len(T), np.int32), np.zeros(len(T))
    for s in range(0, len(T), chunk):
        t = T[s:s + chunk]
        d = [(((t[:, r, 0, None] * x + t[:, r, 1, None] * y) + t[:, r, 2, None] * z) + t[:, r, 3, None]) - dst[None, :, r]
             for r in range(3)]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        inl = d2 < thr2
        count[s:s + chunk] = inl.sum(1)
        err2[s:s + chunk] = np.cumsum(np.where(inl, d2, 0.0), 1)[:, -1] if d2.shape[1] else 0.0
    return count, err2


def better(c1, e1, h1, c2, e2, h2):
    """The total order of the winner: larger count, then smaller err2, then smaller h."""
    return c1 > c2 or (c1 == c2 and (e1 < e2 or (e1 == e2 and h1 < h2)))


def ransac(src, dst, threshold, k=6, iterations=100_000, seed=0):
    """-> {"count" int32 [H], "err2" [H] (+inf where rejected), "ratio" [H] (d2 / d1 of each sample's covariance), "T" [H,4,4],
    "index" (the winner, -1 when there is none), "transform" (its T, else the identity)}."""
    src, dst = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(dst, np.float64).reshape(-1, 3)
    n, H = len(src), int(iterations)
    if n < k or H == 0:
        T = np.tile(np.eye(4), (H, 1, 1))
        return {"count": np.zeros(H, np.int32), "err2": np.full(H, np.inf), "ratio": np.zeros(H), "T": T, "index": -1,
                "transform": np.eye(4)}
    idx = samples(seed, H, n, k)
    T, ok, ratio = umeyama_pairs(src[idx], dst[idx])
    count, err2 = score(src, dst, T, threshold)
    count[~ok] = 0
    err2[~ok] = np.inf
    order = np.lexsort((np.arange(H), err2, -count.astype(np.int64)))
    best = int(order[0])
    if not ok[best]:
        return {"count": count, "err2": err2, "ratio": ratio, "T": T, "index": -1, "transform": np.eye(4)}
    return {"count": count, "err2": err2, "ratio": ratio, "T": T, "index": best, "transform": T[best]}


def similarity_data(n, threshold, seed, outlier_frac=0.4, offset=0.0, extent=1.0):
    """Correspondences under a random similarity (scale 0.3 .. 3, any rotation, a shift of up to 2 extents): src uniform in a
    cube of half side ``extent`` around ``offset``; dst = S src + N(0, 1e-3 threshold) per coordinate; ``outlier_frac`` of the
    targets moved by 10 to 30 thresholds in a random direction.  -> (src, dst, S 4x4, inlier mask)."""
    rs = np.random.RandomState(seed)
    src = offset + rs.uniform(-extent, extent, (n, 3))
    q, _ = np.linalg.qr(rs.randn(3, 3))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    S = np.eye(4)
    S[:3, :3] = rs.uniform(0.3, 3.0) * q
    S[:3, 3] = rs.uniform(-2.0, 2.0, 3) * extent
    dst = src @ S[:3, :3].T + S[:3, 3] + rs.randn(n, 3) * (1e-3 * threshold)
    out = np.zeros(n, bool)
    out[rs.choice(n, int(round(outlier_frac * n)), replace=False)] = True
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dst[out] += u[out] * rs.uniform(10.0, 30.0, (int(out.sum()), 1)) * threshold
    return src, dst, S, ~out
