"""The numpy restatement of rules S and C of the photometric score (include/cds_mvsnet_hip.h) on top of render_ref
and texture_ref, and the cases the photo tests use.  Decisions are integers, everything else fp64 with the bracketing of the rules:
numpy does one IEEE operation per ufunc call and never contracts, so the GPU kernels are expected to agree bit for bit."""
import functools
import math

import numpy as np

import render_ref as R
import texture_ref as T

WIN = 11
C1, C2 = 6.5025, 58.5225
TILE = 16                                                           # CDS_PHOTO_TILE: the side of the compare kernel's tiles


def gauss_table():
    """The window's weights: exp(-(i - 5)^2 / 4.5), divided by their sum in ascending order -> float64 [11]."""
    g = [math.exp(-((i - 5) ** 2) / 4.5) for i in range(WIN)]
    s = 0.0
    for v in g:
        s += v
    return np.array([v / s for v in g], np.float64)


# -------------------------------------------------------------------------------------------------------------------- rule S
def _cell_sample(t, o, c):
    """One coordinate of rule S inside the cells [o, o + c) -> (lo, hi int64, f fp64, clamped bool)."""
    low, high = o.astype(np.float64) + 0.5, (o + c).astype(np.float64) - 0.5
    with np.errstate(invalid="ignore"):
        above = t > low                                             # a NaN takes the lower bound
    tc = np.where(above, t, low)
    below = tc < high
    tc = np.where(below, tc, high)
    x = tc - 0.5
    xl = np.floor(x)
    lo = xl.astype(np.int64)
    return lo, np.minimum(lo + 1, o + c - 1), x - xl, ~above | ~below


def shade_view(vertices, faces, uv, atlas, cam, face_map, with_clamp=False):
    """Rule S for one view: face_map int32 [h,w] -> image uint8 [h,w,3] (and, with_clamp, the pixels whose texel coordinate was
    clamped into its cell, bool [h,w])."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    uv = np.asarray(uv, np.int64).reshape(-1, 3, 2)
    nv = len(np.asarray(vertices).reshape(-1, 3))
    h, w = face_map.shape
    image = np.zeros((h * w, 3), np.uint8)
    clamp = np.zeros(h * w, bool)
    fm = np.asarray(face_map, np.int64).reshape(-1)
    ok = (fm >= 0) & (fm < len(f))
    p = np.nonzero(ok)[0]
    if len(p) and atlas.size:
        win = fm[p]
        keep = ((f[win] >= 0) & (f[win] < nv)).all(1)
        ua, ub = uv[win, 0], uv[win, 1]
        x0, y0, c = ua[:, 0] - 1, ua[:, 1] - 1, ub[:, 0] - ua[:, 0] + 2
        H, W = atlas.shape[:2]
        keep &= (c >= 4) & (x0 >= 0) & (y0 >= 0) & (x0 + c <= W) & (y0 + c <= H)
        p, win, x0, y0, c = p[keep], win[keep], x0[keep], y0[keep], c[keep]
    else:
        p = p[:0]
    if len(p):
        _, _, _, Xc = R.project(vertices, cam)
        n, d = R._planes(Xc, f)
        n, d = n[win], d[win]
        rx, ry = R._rays(cam, p % w, p // w)
        with np.errstate(all="ignore"):
            zf = d / ((n[:, 0] * rx + n[:, 1] * ry) + n[:, 2])
            P = np.stack([zf * rx, zf * ry, zf], 1)
            a, b, cc = (Xc[f[win, k]] - P for k in range(3))
            nn = R._dot(n, n)
            wa, wb, wc = R._dot(n, R._cross(b, cc)) / nn, R._dot(n, R._cross(cc, a)) / nn, R._dot(n, R._cross(a, b)) / nn
            U = uv[win].astype(np.float64)
            tx = (wa * U[:, 0, 0] + wb * U[:, 1, 0]) + wc * U[:, 2, 0]
            ty = (wa * U[:, 0, 1] + wb * U[:, 1, 1]) + wc * U[:, 2, 1]
        xl, xh, fx, cx = _cell_sample(tx, x0, c)
        yl, yh, fy, cy = _cell_sample(ty, y0, c)
        gx, gy = 1.0 - fx, 1.0 - fy
        A = atlas.astype(np.float64)
        for ch in range(3):
            val = (((gx * gy) * A[yl, xl, ch] + (fx * gy) * A[yl, xh, ch]) + (gx * fy) * A[yh, xl, ch]) + (fx * fy) * A[yh, xh, ch]
            image[p, ch] = np.floor(val + 0.5).astype(np.uint8)
        clamp[p] = cx | cy
    image = image.reshape(h, w, 3)
    return (image, clamp.reshape(h, w)) if with_clamp else image


def shade(vertices, faces, uv, atlas, cams, face_maps):
    """Every view -> uint8 [V,h,w,3]."""
    return np.stack([shade_view(vertices, faces, uv, atlas, cam, fm) for cam, fm in zip(cams, face_maps)])


# -------------------------------------------------------------------------------------------------------------------- rule C
def _rows(m, g):
    """((g0 m[:, x'] + g1 m[:, x' + 1]) + ...) + g10 m[:, x' + 10] for every x' -> [h, w - 10]."""
    n = m.shape[1] - WIN + 1
    acc = g[0] * m[:, 0:n]
    for k in range(1, WIN):
        acc = acc + g[k] * m[:, k:k + n]
    return acc


def window_means(m, g):
    """The separable window sum of rule C over the fp64 map m [h,w] -> [h - 10, w - 10]."""
    return _rows(_rows(m, g).T, g).T


def window_counts(mask):
    """mask [h,w] -> bool [h - 10, w - 10]: all 121 bytes of the window are non-zero."""
    ones = np.ones(WIN, np.int64)
    return window_means((np.asarray(mask) != 0).astype(np.int64), ones) == WIN * WIN


def ssim_windows(a, b, g):
    """One channel, a and b uint8 [h,w] with h, w >= 11 -> the ssim of every window, fp64 [h - 10, w - 10]."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    mua, mub = window_means(a, g), window_means(b, g)
    va = window_means(a * a, g) - mua * mua
    vb = window_means(b * b, g) - mub * mub
    vab = window_means(a * b, g) - mua * mub
    return (((2.0 * mua) * mub + C1) * (2.0 * vab + C2)) / (((mua * mua + mub * mub) + C1) * ((va + vb) + C2))


def scores(a, b, mask, g=None):
    """Rule C: a, b uint8 [V,h,w,3], mask uint8 [V,h,w] -> {"n_px" int64 [V], "sse" int64 [V,3], "n_win" int64 [V], "ssim_sum"
    fp64 [V,3] (math.fsum over the counting windows), "ssim_abs" fp64 [V,3] (the sum of |ssim|, for the bound of a sum in any
    order), "ssim_map" fp64 [V,3,max(h-10,0),max(w-10,0)] with NaN where a window does not count, "psnr", "ssim", "coverage"}."""
    g = gauss_table() if g is None else g
    a, b, mask = np.asarray(a, np.uint8), np.asarray(b, np.uint8), np.asarray(mask, np.uint8)
    V, h, w = mask.shape
    mh, mw = max(h - WIN + 1, 0), max(w - WIN + 1, 0)
    if mh == 0 or mw == 0:
        mh = mw = 0
    out = {"n_px": np.zeros(V, np.int64), "sse": np.zeros((V, 3), np.int64), "n_win": np.zeros(V, np.int64),
           "ssim_sum": np.zeros((V, 3)), "ssim_abs": np.zeros((V, 3)), "ssim_map": np.full((V, 3, mh, mw), np.nan)}
    for v in range(V):
        m = mask[v] != 0
        out["n_px"][v] = int(m.sum())
        d = a[v].astype(np.int64) - b[v].astype(np.int64)
        out["sse"][v] = (d * d)[m].sum(0)
        if mh:
            cnt = window_counts(mask[v])
            out["n_win"][v] = int(cnt.sum())
            for ch in range(3):
                s = ssim_windows(a[v, :, :, ch], b[v, :, :, ch], g)
                out["ssim_map"][v, ch] = np.where(cnt, s, np.nan)
                out["ssim_sum"][v, ch] = math.fsum(s[cnt].tolist())
                out["ssim_abs"][v, ch] = math.fsum(np.abs(s[cnt]).tolist())
    out.update(derived(out["n_px"], out["sse"], out["n_win"], out["ssim_sum"], h * w))
    return out


def derived(n_px, sse, n_win, ssim_sum, hw):
    """psnr = 10 log10(255^2 3 n_px / sum sse) (inf at 0 error, NaN at n_px = 0), ssim = sum ssim_sum / (3 n_win) (NaN at 0),
    coverage = n_px / (h w)."""
    with np.errstate(all="ignore"):
        n, e = n_px.astype(np.float64), sse.sum(1).astype(np.float64)
        psnr = np.where(n_px > 0, 10.0 * np.log10((65025.0 * (3.0 * n)) / e), np.nan)
        ssim = np.where(n_win > 0, (ssim_sum[:, 0] + ssim_sum[:, 1] + ssim_sum[:, 2]) / (3.0 * n_win.astype(np.float64)), np.nan)
    return {"psnr": psnr, "ssim": ssim, "coverage": n / float(hw)}


# ------------------------------------------------------------------------------------------------------------------ builders
def grazing_mesh():
    """Four triangles that the camera make_cam(K_SKEW) sees almost edge-on: each reaches 5 to 8 units into the depth, is about
    0.01 pixel high in the image and straddles one row of pixel centres.  Coverage is decided on coordinates snapped to 1/256 pixel, so a
    covered pixel's ray meets the true plane up to a fifth of the triangle away from where the snapped one says: weights outside
    [0, 1], texel coordinates outside the triangle's cell.  wild_mesh() has no such pixel in any of its views."""
    fy, cy = R.K_SKEW[1, 1], R.K_SKEW[1, 2]
    v, f = [], []
    for i, (row, d, e) in enumerate([(24, 0.0039, 0.0047), (30, 0.0061, 0.0029), (36, 0.011, 0.013), (12, 0.0021, 0.0023)]):
        za, zb, zc = 4.0, 4.0 + 0.05 * i, 9.0 + i
        y = lambda vv, z: (vv - cy) * z / fy
        b = len(v)
        v += [(-1.0 + 0.1 * i, y(row + 0.5 - d, za), za), (1.0, y(row + 0.5 - 0.8 * d, zb), zb), (0.1 * i, y(row + 0.5 + e, zc), zc)]
        f.append((b, b + 2, b + 1))
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def shade_case(name, n_views=1, h=R.H, w=R.W):
    """(vertices, colors, faces, images, cams, face maps of the restatement) of a named case; not to be modified.  "plane",
    "sphere", "clutter" and "wild" are the cases of render_ref.reference, "grazing" the mesh above, and "t:<name>" is texture_ref.case(<name>): "t:wild" and "t:plane"
    look at the cameras, "t:special" has the corner face."""
    if name in ("plane", "sphere", "clutter", "wild"):
        v, f, c, cams, maps = R.reference(name, n_views, h, w)
        return v, c, f, T.view_images(n_views, h, w), cams, maps["face"]
    if name == "grazing":
        v, f = grazing_mesh()
        c, images, cams = R.vertex_colors(len(v)), T.view_images(n_views, h, w), R.make_cam(R.K_SKEW)[None].repeat(n_views, 0)
    else:
        v, c, f, images, cams = T.case(name[2:], n_views, h, w)
    return v, c, f, images, cams, R.render(v, f, cams, h, w)["face"]


@functools.lru_cache(maxsize=None)
def shade_reference(name, n_views=1, h=R.H, w=R.W, scale=1.0, max_cell=256):
    """(texture outputs of the restatement, shaded images uint8 [V,h,w,3], clamped pixels bool [V,h,w]) of shade_case(name, ...);
    computed once, not to be modified."""
    v, c, f, images, cams, face = shade_case(name, n_views, h, w)
    tex = T.texture(v, c, f, images, cams, scale, max_cell)
    both = [shade_view(v, f, tex["uv"], tex["atlas"], cam, fm, with_clamp=True) for cam, fm in zip(cams, face)]
    return tex, np.stack([i for i, _ in both]), np.stack([k for _, k in both])


def image_pair(n_views, h, w, seed=0):
    """Two related images and a mask with a hole: b is a with noise and a shifted block, so SSIM spreads over (-1, 1]."""
    rs = np.random.RandomState(seed + 31)
    a = T.view_images(n_views, h, w, seed)
    noise = rs.randint(-40, 41, a.shape)
    b = np.clip(a.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    b[:, h // 3:, w // 2:] = 255 - b[:, h // 3:, w // 2:]           # negative correlation in a part
    mask = np.full((n_views, h, w), 255, np.uint8)
    mask[:, h // 2, w // 3] = 0                                     # one pixel: the windows around it do not count
    if h > 3 and w > 3:
        mask[:, 1, w - 2] = 0
    return a, b, mask


# ------------------------------------------------------------------------------------------------------------------ quality
def holdout_plane(offset=0.0, h=96, w=128, n=3):
    """The analytic-pattern plane of texture_ref seen by five cameras of which view 2 is held out -> (vertices, colors, faces,
    train images, train cams, test image [h,w,3], test cam).  The mesh is plane_mesh(n) with reversed faces, moved by ``offset``
    along z (nearly its normal); the images show the plane where it is, so a moved mesh is textured and rendered with parallax.
    The vertex colours are the pattern at the unmoved vertices, as a fusion of every view would give them."""
    v, f = R.plane_mesh(n)
    f = T.reversed_faces(f)
    K = np.array([[120.0, 0.0, w / 2.0], [0.0, 120.0, h / 2.0], [0.0, 0.0, 1.0]])
    cams = np.stack([R.make_cam(K, R.rot_y(0.25 * (k - 2)) @ R.rot_x(0.1 * (k - 2)), (0.3 * (k - 2), -0.1 * (k - 2), 5.0)) for k in range(5)])
    images = T.plane_images(cams, h, w)
    col = np.floor(np.clip(T.pattern(v.astype(np.float64)), 0, 255) + 0.5).astype(np.uint8)
    moved = v.copy()
    moved[:, 2] += np.float32(offset)
    train = [0, 1, 3, 4]
    return moved, col, np.ascontiguousarray(f, np.int32), images[train], cams[train], images[2], cams[2]


def holdout_scores(offset=0.0, colors="texture"):
    """Held-out PSNR / SSIM of the plane above: textured from four views, rendered into the fifth, compared under valid."""
    v, c, f, images, cams, test, cam = holdout_plane(offset)
    h, w = test.shape[:2]
    maps = R.render(v, f, cam[None], h, w, c)
    if colors == "texture":
        tex = T.texture(v, c, f, images, cams)
        img = shade_view(v, f, tex["uv"], tex["atlas"], cam, maps["face"][0])[None]
    else:
        img = maps["image"]
    return scores(img, test[None], maps["valid"])
