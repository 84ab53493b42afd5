"""Brute-force numpy restatement of the outlier filters of DESIGN §1.16 (csrc/cloud_outlier.hip, pointcloud.remove_outliers):
every number formed with the operations, the precisions and the order that include/cds_mvsnet_hip.h states, so that the GPU
results can be compared bit for bit.  O(M N) memory per block of queries; meant for a few thousand points."""
import numpy as np

CHUNK, LANES = 4096, 256


def pair_d2(query, target):
    """d2 [M,N] float32 = (dx*dx + dy*dy) + dz*dz with d = target - query, every operation rounded to float32."""
    q = np.asarray(query, np.float32)[:, None, :]
    t = np.asarray(target, np.float32)[None, :, :]
    d = t - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn_mean(query, target, k, max_dist=np.inf):
    """-> (mean float64 [M], kth float32 [M]).  The k smallest d2 (a sort), accepted while d2 < max_dist^2 (float32 product);
    terms = k, or min(k, N) for an infinite max_dist; sqrt in float64, summed in ascending order from 0, missing terms count
    as float64(max_dist); one divide."""
    cap = np.float32(max_dist)
    with np.errstate(over="ignore"):
        cap2 = np.float32(cap * cap)
    d2 = np.sort(pair_d2(query, target), axis=1)[:, :k]
    m, n = d2.shape[0], np.asarray(target).shape[0]
    terms = min(k, n) if np.isinf(cap) else k
    accepted = (d2 < cap2).sum(1)                     # a prefix of the sorted row
    s = np.zeros(m, np.float64)
    for j in range(terms):                            # term j of every query at once; the order within a query is j = 0, 1, ...
        t = np.sqrt(d2[:, j].astype(np.float64)) if j < d2.shape[1] else np.full(m, np.float64(cap))
        s = s + np.where(j < accepted, t, np.float64(cap))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s / np.float64(terms)
    kth = np.full(m, cap, np.float32)
    if 0 < terms <= d2.shape[1]:
        full = accepted == terms
        kth[full] = np.sqrt(d2[full, terms - 1])      # float32 sqrt of the largest accepted d2
    return mean, kth


def radius_count(query, target, radius, cap):
    """-> int32 [M]: min(number of targets with d2 <= radius^2 (float32 product), cap)."""
    r = np.float32(radius)
    return np.minimum((pair_d2(query, target) <= np.float32(r * r)).sum(1), cap).astype(np.int32)


def fixed_sum(x):
    """The sum S of cds_outlier_stats_f64: chunks of 4096 terms padded with +0.0; lane l of 256 adds terms l, l + 256, ... to
    +0.0 in that order; the lanes fold by halves (128, 64, ..., 1); the chunk sums are added to +0.0 in ascending order."""
    x = np.asarray(x, np.float64)
    chunks = (x.size + CHUNK - 1) // CHUNK
    a = np.zeros(chunks * CHUNK, np.float64)
    a[:x.size] = x
    a = a.reshape(chunks, CHUNK // LANES, LANES)
    lane = np.zeros((chunks, LANES), np.float64)
    for r in range(CHUNK // LANES):
        lane = lane + a[:, r]
    s = LANES // 2
    while s >= 1:
        lane = lane[:, :s] + lane[:, s:2 * s]
        s //= 2
    total = np.float64(0.0)
    for c in range(chunks):
        total = total + lane[c, 0]
    return total


def stats(x):
    """-> (mu, sigma) float64: mu = S(x) / n, sigma = sqrt(S((x - mu)^2) / (n - 1)), 0 for n = 1."""
    x = np.asarray(x, np.float64)
    n = x.size
    mu = fixed_sum(x) / np.float64(n)
    d = x - mu
    sigma = np.sqrt(fixed_sum(d * d) / np.float64(n - 1)) if n > 1 else np.float64(0.0)
    return mu, sigma


def default_cell(points):
    """pointcloud.default_cell for a numpy cloud (the extent is taken in float32, as torch.aminmax does)."""
    p = np.asarray(points, np.float32)
    e = sorted((p.max(0) - p.min(0)).astype(np.float64).tolist())
    area = max(e[1] * e[2], 1e-12)
    return max(2.0 * np.sqrt(area / max(p.shape[0], 1)), 1e-6 * max(e[2], 1.0))


def remove_outliers(points, nb_neighbors=0, std_ratio=2.0, radius=0.0, min_neighbors=0, max_dist=None):
    """-> (keep bool [N], info).  Statistical: m_i of the cloud against itself with k = nb_neighbors + 1, kept iff
    m_i <= mu + std_ratio * sigma.  Radius: kept iff min_neighbors + 1 points (itself included) lie within radius.  Both rules
    see the input cloud."""
    p = np.asarray(points, np.float32)
    keep = np.ones(p.shape[0], bool)
    info = {"mu": None, "sigma": None, "threshold": None, "removed_statistical": 0, "removed_radius": 0, "mean": None}
    if p.shape[0] and nb_neighbors > 0:
        cap = 16.0 * default_cell(p) if max_dist is None else float(max_dist)
        mean = knn_mean(p, p, nb_neighbors + 1, cap)[0]
        mu, sigma = stats(mean)
        t = float(mu) + float(std_ratio) * float(sigma)
        ok = mean <= t
        info.update(mu=float(mu), sigma=float(sigma), threshold=t, removed_statistical=int((~ok).sum()), mean=mean)
        keep &= ok
    if p.shape[0] and radius > 0:
        ok = radius_count(p, p, radius, min_neighbors + 1) >= min_neighbors + 1
        info["removed_radius"] = int((~ok).sum())
        keep &= ok
    return keep, info


def planted_sphere(seed, n_in=3000, n_out=100):
    """3000 points on the unit sphere with 0.2 % radial noise plus 100 uniform points of [-2, 2]^3 at least 0.3 from the
    sphere, shuffled.  -> (points float32 [3100,3], is_outlier bool [3100])."""
    rs = np.random.RandomState(seed)
    v = rs.randn(n_in, 3)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v *= (1.0 + 0.002 * rs.randn(n_in, 1))
    out = []
    while len(out) < n_out:
        c = rs.uniform(-2.0, 2.0, 3)
        if abs(np.linalg.norm(c) - 1.0) >= 0.3:
            out.append(c)
    pts = np.concatenate([v, np.array(out)]).astype(np.float32)
    flag = np.concatenate([np.zeros(n_in, bool), np.ones(n_out, bool)])
    perm = rs.permutation(len(pts))
    return pts[perm], flag[perm]
