"""The numpy restatement of the texturing rule (include/cds_mvsnet_hip.h) on top of render_ref.render, and the meshes,
images and the analytic pattern the texture tests use.  Decisions are integers, everything else fp64 with the bracketing of the rule:
numpy does one IEEE operation per ufunc call and never contracts, so the GPU kernels are expected to agree bit for bit."""
import functools

import numpy as np

import render_ref as R

ALL = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------------ the rule
def count_votes(face, valid, n_faces):
    """Rule 1: face int32, valid uint8 [V,h,w] -> votes int64 [V,NF]."""
    out = np.zeros((len(face), n_faces), np.int64)
    for v in range(len(face)):
        f = face[v][(valid[v] != 0) & (face[v] >= 0) & (face[v] < n_faces)]
        out[v] = np.bincount(f, minlength=n_faces)
    return out


def best_view(votes, min_px=1):
    """Rule 2: votes [V,NF] -> view int32 [NF], -1 for a face that is not seen."""
    votes = np.asarray(votes, np.int64)
    key = np.zeros(votes.shape[1], np.uint64)
    for v in range(votes.shape[0]):
        key = np.maximum(key, (votes[v].astype(np.uint64) << np.uint64(32)) | (ALL - np.uint64(v)))
    seen = (key >> np.uint64(32)).astype(np.int64) >= min_px
    return np.where(seen, (ALL - (key & ALL)).astype(np.int64), -1).astype(np.int32)


def cell_sizes(vertices, faces, cams, view, scale=1.0, max_cell=256):
    """Rule 3 -> c int32 [NF]."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    c = np.full(len(f), 4, np.int32)
    s2 = np.float64(scale) * np.float64(scale)
    for v in np.unique(view[view >= 0]):
        X, Y, usable, _ = R.project(vertices, cams[v])
        ids = np.nonzero((view == v) & usable[f].all(1))[0]
        Xf, Yf = X[f[ids]], Y[f[ids]]
        L2 = np.zeros(len(ids), np.int64)
        for a in range(3):
            b = (a + 1) % 3
            dx, dy = Xf[:, b] - Xf[:, a], Yf[:, b] - Yf[:, a]
            L2 = np.maximum(L2, dx * dx + dy * dy)
        t = s2 * L2.astype(np.float64)
        cc = np.full(len(ids), max_cell, np.int32)
        p = max_cell // 2
        while p >= 4:                                               # descending: the smallest p that holds wins
            m = np.float64(256.0 * (p - 2))
            cc = np.where(m * m >= t, p, cc)
            p //= 2
        c[ids] = cc
    return c


def _compact(m):
    """The even bits of m, packed (plain Python integers)."""
    out = 0
    for b in range(32):
        out |= ((m >> (2 * b)) & 1) << b
    return out


def pack(c):
    """Rule 4: c [NF] -> (order int64 [NF], starts int64 [NF] by sorted position, total, H, W, origin int32 [NF,2] by face)."""
    c = np.asarray(c, np.int64)
    order = np.argsort(-c, kind="stable")
    units = (c[order] // 4) ** 2
    ends = np.cumsum(units)
    starts = ends - units
    total = int(ends[-1]) if len(c) else 0
    W = 4
    while (W // 4) ** 2 < total:
        W *= 2
    H = W // 2 if 2 * total <= (W // 4) ** 2 else W
    origin = np.zeros((len(c), 2), np.int32)
    for k, f in enumerate(order):
        s = int(starts[k])
        origin[f] = (4 * _compact(s), 4 * _compact(s >> 1))
    return order, starts, total, H, W, origin


def corner_uv(origin, c):
    """Rule 5 -> int32 [NF,3,2]."""
    x0, y0, c = origin[:, 0].astype(np.int64), origin[:, 1].astype(np.int64), np.asarray(c, np.int64)
    return np.stack([np.stack([x0 + 1, y0 + 1], 1), np.stack([x0 + c - 1, y0 + 1], 1), np.stack([x0 + 1, y0 + c - 1], 1)], 1).astype(np.int32)


def _project(cam, P):
    """Rule 1 of the rasteriser for fp64 points [N,3] -> u, v, z."""
    Rm, t, fx, s, cx, fy, cy = R.camera_entries(cam)
    with np.errstate(all="ignore"):
        Xc = [((Rm[r, 0] * P[:, 0] + Rm[r, 1] * P[:, 1]) + Rm[r, 2] * P[:, 2]) + t[r] for r in range(3)]
        z = Xc[2]
        u = ((fx * Xc[0] + s * Xc[1]) + cx * z) / z
        v = (fy * Xc[1] + cy * z) / z
    return u, v, z


def fill(vertices, colors, faces, images, cams, view, c, origin, H, W):
    """Rule 6 -> atlas uint8 [H,W,3].  images: one [h,w,3] array per view; the views may differ in size."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = np.asarray(vertices, np.float32).astype(np.float64)
    col = np.asarray(colors, np.uint8).astype(np.float64)
    atlas = np.zeros((H, W, 3), np.uint8)
    c = np.asarray(c, np.int64)
    # every texel of every cell: its face, i, j
    n = c * c
    face = np.repeat(np.arange(len(f)), n)
    k = np.arange(len(face)) - np.repeat(np.cumsum(n) - n, n)
    i, j = k % c[face], k // c[face]
    den = (c[face] - 2).astype(np.float64)
    wb = ((i.astype(np.float64) + 0.5) - 1.0) / den
    wc = ((j.astype(np.float64) + 0.5) - 1.0) / den
    wa = (1.0 - wb) - wc
    with np.errstate(all="ignore"):
        rgb = np.zeros((len(face), 3), np.float64)
        for ch in range(3):
            val = (wa * col[f[face, 0], ch] + wb * col[f[face, 1], ch]) + wc * col[f[face, 2], ch]
            val = np.where(val > 0, np.where(val < 255, val, 255.0), 0.0)
            rgb[:, ch] = np.floor(val + 0.5)
        P = np.stack([(wa * V[f[face, 0], d] + wb * V[f[face, 1], d]) + wc * V[f[face, 2], d] for d in range(3)], 1)
        for v in np.unique(view[view >= 0]):
            h, w = images[v].shape[:2]                               # the view's own image
            sel = np.nonzero(view[face] == v)[0]
            u, vv, z = _project(cams[v], P[sel])
            ok = (z > 0) & np.isfinite(u) & np.isfinite(vv)
            sel, u, vv = sel[ok], u[ok], vv[ok]
            x = np.minimum(np.maximum(u, 0.5), w - 0.5) - 0.5
            y = np.minimum(np.maximum(vv, 0.5), h - 0.5) - 0.5
            xl, yl = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
            xh, yh = np.minimum(xl + 1, w - 1), np.minimum(yl + 1, h - 1)
            fx, fy = x - xl, y - yl
            gx, gy = 1.0 - fx, 1.0 - fy
            img = images[v].astype(np.float64)
            for ch in range(3):
                val = (((gx * gy) * img[yl, xl, ch] + (fx * gy) * img[yl, xh, ch]) + (gx * fy) * img[yh, xl, ch]) + (fx * fy) * img[yh, xh, ch]
                rgb[sel, ch] = np.floor(val + 0.5)
    atlas[origin[face, 1] + j, origin[face, 0] + i] = rgb.astype(np.uint8)
    return atlas


def texture(vertices, colors, faces, images, cams, scale=1.0, max_cell=256, min_px=1):
    """Rules 1-6 -> {"atlas", "uv", "view", "cell"} as texture.texture_mesh returns them.  images [V,h,w,3] and cams [V,2,4,4], or
    two lists of such arrays, one pair per image size: the views are numbered through the lists."""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    groups = list(zip(images, cams)) if isinstance(images, (list, tuple)) else [(images, cams)]
    votes = []
    for img, cam in groups:
        maps = R.render(vertices, f, cam, img.shape[1], img.shape[2])
        votes.append(count_votes(maps["face"], maps["valid"], len(f)))
    images, cams = [a for img, _ in groups for a in img], np.concatenate([cam for _, cam in groups])
    view = best_view(np.concatenate(votes), min_px)
    c = cell_sizes(vertices, f, cams, view, scale, max_cell)
    _, _, _, H, W, origin = pack(c)
    return {"atlas": fill(vertices, colors, f, images, cams, view, c, origin, H, W), "uv": corner_uv(origin, c), "view": view,
            "cell": np.concatenate([origin, c[:, None].astype(np.int32)], 1)}


# ------------------------------------------------------------------------------------------------------------------ builders
def reversed_faces(f):
    """The same triangles wound the other way."""
    return np.ascontiguousarray(np.asarray(f)[:, ::-1])


def view_images(n, h=R.H, w=R.W, seed=0):
    """n images of h x w: a smooth ramp plus noise, different in every view and every channel."""
    rs = np.random.RandomState(seed + 17)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.zeros((n, h, w, 3), np.uint8)
    for v in range(n):
        for ch in range(3):
            out[v, :, :, ch] = ((3 + v) * x + (5 + ch) * y + 40 * v + rs.randint(0, 60, (h, w))) % 256
    return out


@functools.lru_cache(maxsize=None)
def case(name, n_views=1, h=R.H, w=R.W):
    """(vertices, colors, faces, images, cams) of a named case; not to be modified.  "plane": the plane of render_ref with reversed
    faces, which looks at view_cameras(); "unseen": the same plane as render_ref winds it, which looks away."""
    if name in ("plane", "unseen", "sphere", "wild"):
        v, f = {"plane": R.plane_mesh, "unseen": R.plane_mesh, "sphere": R.uv_sphere, "wild": R.wild_mesh}[name]()
        if name in ("plane", "wild"):
            f = reversed_faces(f)
        cams = R.view_cameras(n_views)
    else:
        v, f = {"clutter": R.clutter_mesh, "special": special_mesh}[name]()
        cams = R.pixel_camera()[None].repeat(n_views, 0)
    return v, R.vertex_colors(len(v)), np.ascontiguousarray(f, np.int32), view_images(n_views, h, w), cams


@functools.lru_cache(maxsize=None)
def special_mesh():
    """For pixel_camera() and a 64 x 48 image, two triangles that look at the camera: one in the image's corner, whose gutter
    texels project to u < 0 and v < 0 (the edge clamp; it also covers pixels of the first column, for an image 1 pixel wide), and
    one from z = 0.05 to z = 5, whose extrapolated texels beyond corner a lie behind the camera (the vertex-colour branch inside a
    seen face)."""
    v = [(0.2, 0.2, 1.0), (20.0, 0.3, 1.0), (0.3, 15.0, 1.0),
         (30.0 * 0.05, 20.0 * 0.05, 0.05), (60.0 * 5.0, 22.0 * 5.0, 5.0), (32.0 * 5.0, 45.0 * 5.0, 5.0)]
    f = [(0, 2, 1), (3, 5, 4)]
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def texel_points(vertices, faces, c):
    """The surface point of every texel of every cell (rule 6) -> face, i, j int64 and P fp64 [N,3]."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = np.asarray(vertices, np.float32).astype(np.float64)
    c = np.asarray(c, np.int64)
    n = c * c
    face = np.repeat(np.arange(len(f)), n)
    k = np.arange(len(face)) - np.repeat(np.cumsum(n) - n, n)
    i, j = k % c[face], k // c[face]
    den = (c[face] - 2).astype(np.float64)
    wb, wc = ((i + 0.5) - 1.0) / den, ((j + 0.5) - 1.0) / den
    wa = (1.0 - wb) - wc
    with np.errstate(all="ignore"):
        P = np.stack([(wa * V[f[face, 0], d] + wb * V[f[face, 1], d]) + wc * V[f[face, 2], d] for d in range(3)], 1)
    return face, i, j, P


@functools.lru_cache(maxsize=None)
def reference(name, n_views=1, h=R.H, w=R.W, scale=1.0, max_cell=256, min_px=1):
    """The restatement's outputs for a named case; computed once, not to be modified."""
    v, c, f, images, cams = case(name, n_views, h, w)
    return texture(v, c, f, images, cams, scale, max_cell, min_px)


# ------------------------------------------------------------------------------------------------------------------ quality
def pattern(P):
    """An analytic colour on world points [N,3] -> fp64 [N,3] in 0..255: several periods across a face of plane_mesh(3)."""
    x, y = P[:, 0], P[:, 1]
    return np.stack([127.5 + 100.0 * np.sin(7.0 * x) * np.cos(5.0 * y), 127.5 + 100.0 * np.cos(6.0 * x + 2.0 * y),
                     127.5 + 100.0 * np.sin(4.0 * y - 3.0 * x)], 1)


def plane_images(cams, h, w):
    """Every view's image of the plane z = 0.3 x - 0.2 y carrying pattern(): the pattern at each pixel centre's intersection."""
    n = np.array([0.3, -0.2, -1.0])
    py, px = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.zeros((len(cams), h, w, 3), np.uint8)
    for v, cam in enumerate(cams):
        Rm, t = R.camera_entries(cam)[:2]
        rx, ry = R._rays(cam, px.ravel(), py.ravel())
        d = np.stack([rx, ry, np.ones_like(rx)], 1) @ Rm                  # R^T r per row
        C = -Rm.T @ t
        lam = -(n @ C) / (d @ n)
        out[v] = np.floor(np.clip(pattern(C + lam[:, None] * d), 0, 255) + 0.5).reshape(h, w, 3).astype(np.uint8)
    return out


def atlas_lookup(atlas, xy):
    """Bilinear lookup at texel coordinates xy [N,2] (texel (x, y) has its centre at (x + 0.5, y + 0.5)) -> fp64 [N,3]."""
    H, W = atlas.shape[:2]
    x, y = np.clip(xy[:, 0] - 0.5, 0, W - 1), np.clip(xy[:, 1] - 0.5, 0, H - 1)
    xl, yl = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    xh, yh = np.minimum(xl + 1, W - 1), np.minimum(yl + 1, H - 1)
    fx, fy = (x - xl)[:, None], (y - yl)[:, None]
    a = atlas.astype(np.float64)
    return (1 - fx) * (1 - fy) * a[yl, xl] + fx * (1 - fy) * a[yl, xh] + (1 - fx) * fy * a[yh, xl] + fx * fy * a[yh, xh]
