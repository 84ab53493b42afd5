"""Float64 numpy restatements of the two rules of DESIGN §1.8 (include/cds_mvsnet_hip.h): the oriented normals of a depth
map (cds_depth_normals_f32) and the merge of a cloud to one attributed point per voxel (cds_voxel_merge_f32).

The normals are restated independently of the kernel's closed form: the window's normal equations go through
``np.linalg.solve``.  Only the decision ``ok`` repeats the rule's own expressions (integer determinant, t = adj(S) b in the
stated order), because the rule fixes it bit for bit."""
import numpy as np

from tt_eval_ref import voxel_keys


def _pixel_valid(depth, valid):
    d = np.asarray(depth)
    v = np.isfinite(d) & (d > 0)
    return v if valid is None else v & (np.asarray(valid) != 0)


def depth_normals(depth, K, E, valid=None, radius=2, jump=0.01, min_pts=6):
    """depth [h,w] (float32, or float64 for the plane-exactness check), K [3,3], E [4,4] -> (normals float64 [3,h,w] before
    the final rounding to float32, ok uint8 [h,w]).  ``jump`` is the float32 the kernel receives."""
    depth = np.asarray(depth)
    h, w = depth.shape
    K = np.asarray(K, np.float64)
    R = np.asarray(E, np.float64)[:3, :3]
    r = int(radius)
    jump = float(np.float32(jump))
    good = _pixel_valid(depth, valid)
    d64 = np.where(good, depth, 1.0).astype(np.float64)
    inv = 1.0 / d64
    normals = np.zeros((3, h, w))
    ok = np.zeros((h, w), np.uint8)
    dys, dxs = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")      # dy outer, dx inner
    dys, dxs = dys.reshape(-1), dxs.reshape(-1)
    for y in range(h):
        for x in range(w):
            if not good[y, x]:
                continue
            dc = d64[y, x]
            qy, qx = y + dys, x + dxs
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx, dy, dx = qy[inside], qx[inside], dys[inside], dxs[inside]
            enter = good[qy, qx] & (np.abs(d64[qy, qx] - dc) <= jump * dc)
            qy, qx, dy, dx = qy[enter], qx[enter], dy[enter], dx[enter]
            n = len(dx)
            v = np.stack([dx, dy, np.ones_like(dx)], 1)                       # [n,3] integers
            S = v.T @ v                                                       # exact
            iv = inv[qy, qx]
            b = np.cumsum(v.astype(np.float64) * iv[:, None], 0)[-1]          # sequential sums in visiting order
            (sxx, sxy, sx), (_, syy, sy) = (int(a) for a in S[0]), (int(a) for a in S[1])
            A = np.array([[syy * n - sy * sy, sx * sy - sxy * n, sxy * sy - syy * sx],
                          [sx * sy - sxy * n, sxx * n - sx * sx, sxy * sx - sxx * sy],
                          [sxy * sy - syy * sx, sxy * sx - sxx * sy, sxx * syy - sxy * sxy]], np.float64)
            det = sxx * int(A[0, 0]) + sxy * int(A[0, 1]) + sx * int(A[0, 2])
            t2 = (A[2, 0] * b[0] + A[2, 1] * b[1]) + A[2, 2] * b[2]
            if n < min_pts or det == 0 or not t2 > 0:
                continue
            g = np.linalg.solve(S.astype(np.float64), b)                      # the affine map pixel offset -> 1 / z
            px, py = x + 0.5, y + 0.5
            g = np.array([g[0], g[1], g[2] - g[0] * px - g[1] * py])
            nw = R.T @ (-(K.T @ g))
            nn = np.linalg.norm(nw)
            if not (np.isfinite(nn) and nn > 0):
                continue
            normals[:, y, x] = nw / nn
            ok[y, x] = 1
    return normals, ok


def merge_voxels(points, colors, voxel, normals=None, min_points=1):
    """points float32 [N,3], colors uint8 [N,3], normals float32 [N,3] | None -> dict(points float32 [V,3], colors uint8
    [V,3], normals float64 [V,3] | None (before the final rounding), counts int64 [V], keys int64 [V]), ascending key order,
    voxels with fewer than ``min_points`` points dropped."""
    p = np.asarray(points, np.float32)
    c = np.asarray(colors, np.uint8).astype(np.int64)
    if len(p) == 0:
        return {"points": np.zeros((0, 3), np.float32), "colors": np.zeros((0, 3), np.uint8),
                "normals": None if normals is None else np.zeros((0, 3)), "counts": np.zeros(0, np.int64),
                "keys": np.zeros(0, np.int64)}
    keys = voxel_keys(p, voxel)
    order = np.argsort(keys, kind="stable")
    ukeys, first, counts = np.unique(keys[order], return_index=True, return_counts=True)
    out_p, out_c, out_n = [], [], []
    for f, k in zip(first, counts):
        idx = order[f:f + k]                                                  # input indices, ascending
        out_p.append((np.cumsum(p[idx].astype(np.float64), 0)[-1] / float(k)).astype(np.float32))
        out_c.append((2 * c[idx].sum(0) + k) // (2 * k))
        if normals is not None:
            s = np.cumsum(np.asarray(normals, np.float32)[idx].astype(np.float64), 0)[-1]
            nn = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
            out_n.append(s / nn if np.isfinite(nn) and nn > 0 else np.zeros(3))
    keep = counts >= int(min_points)
    return {"points": np.stack(out_p)[keep], "colors": np.stack(out_c).astype(np.uint8)[keep],
            "normals": None if normals is None else np.stack(out_n)[keep], "counts": counts.astype(np.int64)[keep],
            "keys": ukeys.astype(np.int64)[keep]}


def tilted_plane(h, w, dtype, n=(0.1, -0.07, 1.0), z0=650.0, f=None):
    """A perspective depth image of the plane n . X = n_z z0 in the camera frame -> (depth [h,w] of ``dtype``, K, E, the unit
    world-frame normal that faces the camera).  E is a fixed non-trivial rotation with a translation."""
    f = float(f if f is not None else 1.2 * w)
    K = np.array([[f, 0.3, w / 2.0 - 0.7], [0.0, 1.07 * f, h / 2.0 + 0.4], [0.0, 0.0, 1.0]])
    a, b = 0.4, -0.25
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    E = np.eye(4)
    E[:3, :3] = Rx @ Ry
    E[:3, 3] = [12.0, -7.0, 30.0]
    n = np.asarray(n, np.float64)
    rho = n[2] * z0
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    rays = np.linalg.inv(K) @ np.stack([xs, ys, np.ones_like(xs)]).reshape(3, -1)          # z = 1
    depth = (rho / (n @ rays)).reshape(h, w)
    nc = -n / np.linalg.norm(n)                                                            # n . ray > 0: flip to face the camera
    return depth.astype(dtype), K, E, E[:3, :3].T @ nc


def angle_deg(normals, ok, true_n):
    """Largest angle in degrees between the ok normals [3,h,w] and the unit vector ``true_n``, from the cross product
    (accurate for tiny angles)."""
    n = normals[:, ok > 0]
    cr = np.linalg.norm(np.cross(n.T, true_n[None, :]), axis=1)
    return float(np.degrees(np.arctan2(cr, n.T @ true_n)).max())
