"""A numpy restatement of the weighted integration rule of DESIGN §1.14 (include/cds_mvsnet_hip.h, "Weighted TSDF fusion"): the
weight map of a view, the depth interpolated between pixels, and the integration that uses both.  fp64 where the rule says fp64,
``np.float32`` adds where it says fp32.  Frame, allocation and extraction are those of mesh_ref.py, unchanged; a volume is
mesh_ref's dict plus ``wn`` int32 [NB,512], the sum of the weights.  Nothing here is shared with the kernels.
"""
from __future__ import annotations

import functools

import numpy as np

import cloud_ref as C
import mesh_ref as M


# ---------------------------------------------------------------------------------------------------------------- weights
def view_weights(depth, mask, K, E, normals=None, ok=None, conf=None) -> np.ndarray:
    """depth float32 [h,w], mask [h,w], K [3,3] and E [4,4] (their float32 values are used), normals float32 [3,h,w] (world
    frame) with ok [h,w] or both None, conf float32 [h,w] or None -> uint8 [h,w]."""
    depth = np.asarray(depth, np.float32)
    h, w = depth.shape
    K = np.asarray(K, np.float32).astype(np.float64)
    R = np.asarray(E, np.float32).astype(np.float64)[:3, :3]
    assert K[1, 0] == 0 and K[2].tolist() == [0.0, 0.0, 1.0]
    assert (normals is None) == (ok is None)
    kept = (np.asarray(mask) != 0) & np.isfinite(depth) & (depth > 0)
    with np.errstate(all="ignore"):
        a = np.ones((h, w))
        if normals is not None:
            n = np.asarray(normals, np.float32).astype(np.float64)
            ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
            c1 = ((ys + 0.5) - K[1, 2]) / K[1, 1]
            c0 = (((xs + 0.5) - K[0, 2]) - K[0, 1] * c1) / K[0, 0]
            nc = [(R[r, 0] * n[0] + R[r, 1] * n[1]) + R[r, 2] * n[2] for r in range(3)]
            a = -((nc[0] * c0 + nc[1] * c1) + nc[2]) / np.sqrt((c0 * c0 + c1 * c1) + 1.0)
            a = np.where(np.isfinite(a) & (a >= 0), np.minimum(a, 1.0), 0.0)
            a = np.where(np.asarray(ok) != 0, a, 0.0)
        c = np.ones((h, w))
        if conf is not None:
            cf = np.asarray(conf, np.float32).astype(np.float64)
            c = np.where(cf >= 0, np.minimum(cf, 1.0), 0.0)                   # NaN fails the comparison
        wt = np.floor(255.0 * (a * c) + 0.5)
    return np.where(kept, np.clip(wt, 1, 255), 0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------- interpolation
def quad_state(depth, mask, jump):
    """Every quad of four neighbouring pixels of a map, by its upper left pixel: int [h-1,w-1], 0 when its depth is interpolated,
    1 when a corner is not kept (masked, or a depth that is not finite or not > 0), 2 when the corners are more than ``jump``
    (relative to the smallest) apart."""
    d = np.asarray(depth, np.float32)
    kept = (np.asarray(mask) != 0) & np.isfinite(d) & (d > 0)
    corners = [(slice(None, -1), slice(None, -1)), (slice(None, -1), slice(1, None)), (slice(1, None), slice(None, -1)),
               (slice(1, None), slice(1, None))]
    all_kept = np.logical_and.reduce([kept[c] for c in corners])
    with np.errstate(all="ignore"):
        dq = np.stack([np.where(kept, d, 1.0)[c].astype(np.float64) for c in corners])
        lo, hi = dq.min(0), dq.max(0)
        close = hi - lo <= float(np.float32(jump)) * lo
    return np.where(~all_kept, 1, np.where(close, 0, 2))


def interp_depth(depth, mask, u, v, jump):
    """The depth the rule uses at the positions (u, v) (float64 arrays, 0 <= u < w, 0 <= v < h) of a map whose nearest pixel
    (floor(u), floor(v)) is kept -> (dd float64: 1 / i where the quad around the position interpolates, else the nearest pixel's
    depth; took bool: it was interpolated)."""
    d = np.asarray(depth, np.float32)
    h, w = d.shape
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    near = d[np.floor(v).astype(np.int64), np.floor(u).astype(np.int64)].astype(np.float64)
    if h < 2 or w < 2:
        return near, np.zeros(u.shape, bool)
    a, b = u - 0.5, v - 0.5
    x0, y0 = np.floor(a), np.floor(b)
    fx, fy = a - x0, b - y0
    inside = (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
    xi, yi = np.where(inside, x0, 0).astype(np.int64), np.where(inside, y0, 0).astype(np.int64)
    took = inside & (quad_state(d, mask, jump)[yi, xi] == 0)
    with np.errstate(all="ignore"):
        i00, i10 = 1.0 / d[yi, xi].astype(np.float64), 1.0 / d[yi, xi + 1].astype(np.float64)
        i01, i11 = 1.0 / d[yi + 1, xi].astype(np.float64), 1.0 / d[yi + 1, xi + 1].astype(np.float64)
        i0 = i00 + fx * (i10 - i00)
        i1 = i01 + fx * (i11 - i01)
        dd = 1.0 / (i0 + fy * (i1 - i0))
    return np.where(took, dd, near), took


# ------------------------------------------------------------------------------------------------------------ integration
def empty_like(vol: dict) -> dict:
    out = M.empty_volume(vol["origin"], vol["voxel"], vol["trunc"], vol["nb"], vol["keys"])
    out["wn"] = np.zeros_like(out["n"])
    return out


def allocate(points, voxel, trunc) -> dict:
    return empty_like(M.allocate(points, voxel, trunc))


def integrate(vol: dict, depths, masks, images, cams, weights=None, interp=False, jump=0.05) -> None:
    """mesh_ref.integrate with weights uint8 [V,h,w] or None (every kept pixel weighs 1) and the interpolated depth; ``wn`` gets
    the weight of every view that ``n`` counts."""
    X = M.lattice_points(vol).reshape(-1, 3)
    T = vol["trunc"]
    s, n, nc, wn = vol["sum"].reshape(-1), vol["n"].reshape(-1), vol["nc"].reshape(-1), vol["wn"].reshape(-1)
    rgb = vol["rgb"].reshape(3, -1)
    h, w = depths.shape[1:]
    with np.errstate(all="ignore"):
        for v in range(depths.shape[0]):
            E = cams[v, 0].astype(np.float32).astype(np.float64)
            K = cams[v, 1, :3, :3].astype(np.float32).astype(np.float64)
            xc = [((E[r, 0] * X[:, 0] + E[r, 1] * X[:, 1]) + E[r, 2] * X[:, 2]) + E[r, 3] for r in range(3)]
            z = xc[2]
            p = [(K[r, 0] * xc[0] + K[r, 1] * xc[1]) + K[r, 2] * xc[2] for r in range(3)]
            u, vv = p[0] / p[2], p[1] / p[2]
            ok = (z > 0) & (u >= 0) & (u < w) & (vv >= 0) & (vv < h)
            x = np.where(ok, np.floor(u), 0).astype(np.int64)
            y = np.where(ok, np.floor(vv), 0).astype(np.int64)
            d = depths[v][y, x]
            ok &= (masks[v][y, x] != 0) & np.isfinite(d) & (d > 0)
            wq = weights[v][y, x].astype(np.int32) if weights is not None else np.ones(len(X), np.int32)
            ok &= wq != 0
            dd = d.astype(np.float64)
            if interp:
                dd = interp_depth(depths[v], masks[v], np.where(ok, u, 0.0), np.where(ok, vv, 0.0), jump)[0]
            sdf = dd - z
            ok &= ~(sdf < -T)
            tv = (wq.astype(np.float64) * np.minimum(1.0, sdf / T)).astype(np.float32)
            s[ok] = s[ok] + tv[ok]                       # float32 + float32
            n[ok] += 1
            wn[ok] += wq[ok]
            near = ok & (sdf <= T)
            col = images[v][y, x].astype(np.int32)
            for c in range(3):
                rgb[c][near] += col[near, c]
            nc[near] += 1


def extract(vol: dict, min_weight: int = 2) -> dict:
    """mesh_ref.extract of a weighted volume: a point is valid iff n >= min_weight, its distance is sum / wn.  mesh_ref divides by
    ``n`` and tests it against min_weight, so it gets n := wn where the point is valid and 0 elsewhere, and min_weight 1 (wn >= n:
    a counted view weighs at least 1)."""
    assert (vol["wn"] >= vol["n"]).all()
    return M.extract(dict(vol, n=np.where(vol["n"] >= int(min_weight), vol["wn"], 0).astype(np.int32)), 1)


# ----------------------------------------------------------------------------------------------------------------- scenes
JUMP = 0.05


@functools.lru_cache(maxsize=None)
def sphere_weights():
    """The angle weights of mesh_ref.sphere_scene's 26 views from the normals of cloud_ref.depth_normals (defaults, valid = mask),
    rounded to float32 as the kernel writes them -> (uint8 [26,h,w], share of the kept pixels that have a normal)."""
    sc = M.sphere_case()[0]
    out, with_normal, kept = [], 0, 0
    for v in range(len(sc["depths"])):
        K, E = sc["cams"][v, 1, :3, :3], sc["cams"][v, 0]
        nrm, ok = C.depth_normals(sc["depths"][v], K, E, valid=sc["masks"][v])
        out.append(view_weights(sc["depths"][v], sc["masks"][v], K, E, nrm.astype(np.float32), ok))
        with_normal += int(ok.sum())
        kept += int((sc["masks"][v] != 0).sum())
    return np.stack(out), with_normal / kept


@functools.lru_cache(maxsize=None)
def sphere_mode(weighted: bool, interp: bool):
    """(integrated volume, mesh) of the sphere scene with T = 2.5 voxels and min_weight 2 in one of the four modes; computed
    once, not to be modified."""
    sc = M.sphere_case()[0]
    vol = allocate(sc["points"], sc["voxel"], 2.5 * sc["voxel"])
    integrate(vol, sc["depths"], sc["masks"], sc["images"], sc["cams"], sphere_weights()[0] if weighted else None, interp, JUMP)
    return vol, extract(vol, 2)


def radial_error(vertices, sc):
    """(rms, max) of | |v - centre| - r | over the vertices, in voxels."""
    e = np.abs(np.linalg.norm(np.asarray(vertices, np.float64) - sc["centre"], axis=1) - sc["radius"]) / sc["voxel"]
    return float(np.sqrt((e * e).mean())), float(e.max())


def scene_weights(sc, seed=0):
    """Seeded random weights uint8 [V,h,w] for an integration_scene: a quarter of them 0, some 1 and 255."""
    rs = np.random.RandomState(500 + seed)
    wt = rs.randint(0, 256, sc["depths"].shape).astype(np.uint8)
    wt[rs.rand(*wt.shape) < 0.25] = 0
    wt[rs.rand(*wt.shape) < 0.05] = 1
    wt[rs.rand(*wt.shape) < 0.05] = 255
    return wt


@functools.lru_cache(maxsize=None)
def integration_case(n_views: int, trunc_voxels: float, weighted: bool, interp: bool):
    """(scene, weights or None, integrated volume) of mesh_ref.integration_scene; computed once, not to be modified."""
    sc = M.integration_case(n_views, trunc_voxels)[0]
    wt = scene_weights(sc) if weighted else None
    vol = allocate(sc["points"], sc["voxel"], trunc_voxels * sc["voxel"])
    integrate(vol, sc["depths"], sc["masks"], sc["images"], sc["cams"], wt, interp, JUMP)
    return sc, wt, vol
