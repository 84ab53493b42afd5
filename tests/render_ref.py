"""The numpy restatement of the mesh rendering rule (include/cds_mvsnet_hip.h), and the meshes and cameras the
render tests use.  Decisions are int64, everything else fp64 with the bracketing of the rule: numpy does one IEEE operation per
ufunc call and never contracts, so the GPU kernels are expected to agree bit for bit."""
import functools

import numpy as np

SNAP_LIMIT = 1 << 28
MISS = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------------ the rule
def camera_entries(cam):
    """cam [2,4,4] float32 -> (R [3,3], t [3], fx, s, cx, fy, cy) as fp64 of the fp32 entries."""
    cam = np.asarray(cam, np.float32).astype(np.float64)
    K = cam[1, :3, :3]
    if K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1:
        raise ValueError("K must be [[fx, s, cx], [0, fy, cy], [0, 0, 1]]")
    return cam[0, :3, :3], cam[0, :3, 3], K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]


def project(vertices, cam):
    """Rule 1 -> X, Y int64 [NV] (0 where unusable), usable bool [NV], Xc fp64 [NV,3]."""
    R, t, fx, s, cx, fy, cy = camera_entries(cam)
    V = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        Xc = np.stack([((R[r, 0] * V[:, 0] + R[r, 1] * V[:, 1]) + R[r, 2] * V[:, 2]) + t[r] for r in range(3)], 1)
        z = Xc[:, 2]
        u = ((fx * Xc[:, 0] + s * Xc[:, 1]) + cx * z) / z
        v = (fy * Xc[:, 1] + cy * z) / z
        sx, sy = np.floor(u * 256.0 + 0.5), np.floor(v * 256.0 + 0.5)
        usable = (z > 0) & np.isfinite(u) & np.isfinite(v) & (np.abs(sx) < SNAP_LIMIT) & (np.abs(sy) < SNAP_LIMIT)
    X = np.where(usable, sx, 0.0).astype(np.int64)
    Y = np.where(usable, sy, 0.0).astype(np.int64)
    return X, Y, usable, Xc


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _planes(Xc, f):
    """Rule 4 per face: n [NF,3], d [NF]."""
    a, b, c = Xc[f[:, 0]], Xc[f[:, 1]], Xc[f[:, 2]]
    with np.errstate(all="ignore"):                                 # faces with a vertex at infinity: never drawn
        n = _cross(b - a, c - a)
        return n, _dot(n, a)


def _rays(cam, px, py):
    _, _, fx, s, cx, fy, cy = camera_entries(cam)
    ry = ((py.astype(np.float64) + 0.5) - cy) / fy
    rx = (((px.astype(np.float64) + 0.5) - cx) - s * ry) / fx
    return rx, ry


def fragments(vertices, faces, cam, h, w):
    """Rules 1-4: every fragment of one view -> {"face", "px", "py" int64, "zf" fp64, "front" bool}, in face order."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    X, Y, usable, Xc = project(vertices, cam)
    empty = {k: np.zeros(0, np.int64) for k in ("face", "px", "py")}
    empty.update(zf=np.zeros(0), front=np.zeros(0, bool))
    if len(f) == 0:
        return empty
    Xf, Yf = X[f], Y[f]
    A = (Xf[:, 1] - Xf[:, 0]) * (Yf[:, 2] - Yf[:, 0]) - (Yf[:, 1] - Yf[:, 0]) * (Xf[:, 2] - Xf[:, 0])
    drawn = usable[f].all(1) & (A != 0)
    g = np.sign(A)
    px0 = np.maximum(0, (Xf.min(1) - 128 + 255) >> 8)
    px1 = np.minimum(w - 1, (Xf.max(1) - 128) >> 8)
    py0 = np.maximum(0, (Yf.min(1) - 128 + 255) >> 8)
    py1 = np.minimum(h - 1, (Yf.max(1) - 128) >> 8)
    bw = np.where(drawn, np.maximum(px1 - px0 + 1, 0), 0)
    bh = np.where(drawn, np.maximum(py1 - py0 + 1, 0), 0)
    cnt = bw * bh
    ids = np.nonzero(cnt)[0]
    if len(ids) == 0:
        return empty
    face = np.repeat(ids, cnt[ids])
    i = np.arange(len(face)) - np.repeat(np.cumsum(cnt[ids]) - cnt[ids], cnt[ids])
    px, py = px0[face] + i % bw[face], py0[face] + i // bw[face]
    Qx, Qy = 256 * px + 128, 256 * py + 128
    inside = np.ones(len(face), bool)
    for a in range(3):
        b = (a + 1) % 3
        dx, dy = g[face] * (Xf[face, b] - Xf[face, a]), g[face] * (Yf[face, b] - Yf[face, a])
        E = dx * (Qy - Yf[face, a]) - dy * (Qx - Xf[face, a])
        inside &= (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
    face, px, py = face[inside], px[inside], py[inside]
    n, d = _planes(Xc, f)
    rx, ry = _rays(cam, px, py)
    with np.errstate(all="ignore"):
        zf = d[face] / ((n[face, 0] * rx + n[face, 1] * ry) + n[face, 2])
    ok = np.isfinite(zf) & (zf > 0)
    return {"face": face[ok], "px": px[ok], "py": py[ok], "zf": zf[ok], "front": (d[face] < 0)[ok]}


def render_view(vertices, faces, cam, h, w, colors=None):
    """Rules 1-6 for one view -> {"depth" float32, "face" int32, "front", "valid" uint8 [h,w][, "image" uint8 [h,w,3]]}."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    fr = fragments(vertices, f, cam, h, w)
    keys = np.full(h * w, MISS, np.uint64)
    with np.errstate(all="ignore"):
        bits = fr["zf"].astype(np.float32).view(np.uint32).astype(np.uint64)
    np.minimum.at(keys, fr["py"] * w + fr["px"], (bits << np.uint64(32)) | fr["face"].astype(np.uint64))
    hit = keys != MISS
    out = {"depth": np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).reshape(h, w),
           "face": np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32).reshape(h, w)}
    front = np.zeros(h * w, np.uint8)
    image = np.zeros((h * w, 3), np.uint8)
    p = np.nonzero(hit)[0]
    if len(p):
        win = out["face"].reshape(-1)[p].astype(np.int64)
        _, _, _, Xc = project(vertices, cam)
        n, d = _planes(Xc, f)
        n, d = n[win], d[win]
        front[p] = d < 0
        if colors is not None:
            rx, ry = _rays(cam, p % w, p // w)
            with np.errstate(all="ignore"):
                zf = d / ((n[:, 0] * rx + n[:, 1] * ry) + n[:, 2])
                P = np.stack([zf * rx, zf * ry, zf], 1)
                a, b, c = (Xc[f[win, k]] - P for k in range(3))
                nn = _dot(n, n)
                wa, wb, wc = _dot(n, _cross(b, c)) / nn, _dot(n, _cross(c, a)) / nn, _dot(n, _cross(a, b)) / nn
                col = np.asarray(colors, np.uint8).astype(np.float64)
                for ch in range(3):
                    val = (wa * col[f[win, 0], ch] + wb * col[f[win, 1], ch]) + wc * col[f[win, 2], ch]
                    val = np.where(val > 0, np.where(val < 255, val, 255.0), 0.0)            # NaN -> 0
                    image[p, ch] = np.floor(val + 0.5).astype(np.uint8)
    out["front"] = front.reshape(h, w)
    out["valid"] = front.reshape(h, w).copy()
    if colors is not None:
        out["image"] = image.reshape(h, w, 3)
    return out


def render(vertices, faces, cams, h, w, colors=None):
    """Every view -> arrays [V,h,w(,3)] as render_mesh returns them."""
    views = [render_view(vertices, faces, cam, h, w, colors) for cam in cams]
    names = ["depth", "face", "front", "valid"] + (["image"] if colors is not None else [])
    shapes = {"depth": np.float32, "face": np.int32, "front": np.uint8, "valid": np.uint8, "image": np.uint8}
    return {k: np.stack([v[k] for v in views]) if views else np.zeros((0, h, w) + ((3,) if k == "image" else ()), shapes[k])
            for k in names}


# ------------------------------------------------------------------------------------------------------------------ builders
H, W = 48, 64
K_SKEW = np.array([[60.0, 0.3, 31.7], [0.0, 58.0, 23.9], [0.0, 0.0, 1.0]])
SPHERE_R = 1.3


def make_cam(K, R=np.eye(3), t=(0.0, 0.0, 0.0)):
    cam = np.zeros((2, 4, 4), np.float32)
    cam[0, :3, :3], cam[0, :3, 3], cam[0, 3, 3] = R, t, 1.0
    cam[1, :3, :3], cam[1, 3, 3] = K, 1.0
    return cam


def rot_y(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def rot_x(a):
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])


def view_cameras(n=1):
    """View 0: the skewed K, rotated 0.3 rad about y, t = (0.1, -0.05, 5); the others turn and shift it a little more."""
    return np.stack([make_cam(K_SKEW, rot_x(0.17 * k) @ rot_y(0.3 + 0.23 * k), (0.1 - 0.07 * k, -0.05 + 0.04 * k, 5.0 + 0.3 * k))
                     for k in range(n)])




def pixel_camera():
    """K = 1, E = 1: a vertex (x, y, 1) lands on u = x, v = y exactly."""
    return make_cam(np.eye(3))


def vertex_colors(n):
    i = np.arange(n)
    return np.stack([(37 * i + 11) % 256, (91 * i + 5) % 256, (13 * i + 200) % 256], 1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def plane_mesh(n=9):
    """n x n vertices of z = 0.3 x - 0.2 y over [-2, 2]^2, two triangles per cell."""
    g = np.linspace(-2.0, 2.0, n)
    x, y = np.meshgrid(g, g, indexing="xy")
    v = np.stack([x.ravel(), y.ravel(), (0.3 * x - 0.2 * y).ravel()], 1).astype(np.float32)
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            f += [(a, a + 1, a + n + 1), (a, a + n + 1, a + n)]
    return v, np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def uv_sphere(n_lon=24, n_lat=16, radius=SPHERE_R):
    """A closed sphere around the origin: two poles and n_lat - 1 rings of n_lon vertices, wound counter-clockwise from outside."""
    v = [(0.0, 0.0, radius)]
    for j in range(1, n_lat):
        th = np.pi * j / n_lat
        for i in range(n_lon):
            ph = 2.0 * np.pi * i / n_lon
            v.append((radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)))
    v.append((0.0, 0.0, -radius))
    ring = lambda j, i: 1 + (j - 1) * n_lon + i % n_lon
    south = len(v) - 1
    f = []
    for i in range(n_lon):
        f.append((0, ring(1, i), ring(1, i + 1)))
        for j in range(1, n_lat - 1):
            f += [(ring(j, i), ring(j + 1, i), ring(j + 1, i + 1)), (ring(j, i), ring(j + 1, i + 1), ring(j, i + 1))]
        f.append((south, ring(n_lat - 1, i + 1), ring(n_lat - 1, i)))
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def clutter_mesh(seed=0):
    """Two triangles that span a 64 x 48 map of pixel_camera() at z = 2, and 200 sub-pixel triangles in front of them at z = 1.
    Vertices are (u z, v z, z), so they project to (u, v)."""
    rs = np.random.RandomState(seed)
    v = [(-2.0, -2.0, 2.0), (140.0, -2.0, 2.0), (140.0, 100.0, 2.0), (-2.0, 100.0, 2.0)]
    f = [(0, 2, 1), (0, 2, 3)]                                      # the first looks at the camera, the second away
    for k in range(200):
        c = np.array([rs.uniform(0, 64), rs.uniform(0, 48)])
        for _ in range(3):
            p = c + rs.uniform(-0.8, 0.8, 2)
            v.append((p[0], p[1], 1.0))
        f.append((4 + 3 * k, 5 + 3 * k, 6 + 3 * k))
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def wild_mesh():
    """The plane mesh in front of view_cameras(), plus faces with a vertex behind the camera, at 1e30, non-finite, far outside the
    map but usable (-5e6: its face is clamped to the map) and beyond the 2^28 limit (5e5 along y), a degenerate face, and one large
    face behind the plane that reaches past the map on every side."""
    v, f = plane_mesh()
    n = len(v)
    extra = np.array([[0.0, 0.0, -9.0], [300.0, 1.0, 0.0], [1e30, 0.0, 0.0], [0.0, 1e30, 1e30], [np.inf, 0.0, 0.0], [np.nan, 0.0, 0.0],
                      [-12.0, -30.0, 1.0], [12.0, -30.0, 1.0], [0.0, 60.0, 1.0], [-5e6, 0.0, 0.0], [0.0, 5e5, 0.0]], np.float32)
    ef = [(0, 1, n), (2, n + 1, 3), (4, 5, n + 2), (6, n + 3, 7), (8, 9, n + 4), (10, n + 5, 11), (12, 12, 13), (n + 6, n + 7, n + 8),
          (0, 40, 80), (20, 21, n + 9), (30, n + 10, 31)]
    return np.concatenate([v, extra]), np.concatenate([f, np.asarray(ef, np.int32)])


@functools.lru_cache(maxsize=None)
def last_bit_mesh():
    """Pairs of parallel triangles seen by pixel_camera() whose depths differ in the last fp32 bit; the nearer one has the HIGHER
    face index in every second pair."""
    v, f = [], []
    for k in range(8):
        z0 = np.float32(1.0 + 0.37 * k)
        z1 = np.nextafter(z0, np.float32(9.0))
        near_first = k % 2 == 0
        for z in ((z0, z1) if near_first else (z1, z0)):
            b = len(v)
            x0, y0 = 2.0 + 6.0 * k, 3.0
            v += [(x0 * z, y0 * z, z), ((x0 + 5.0) * z, y0 * z, z), (x0 * z, (y0 + 9.0) * z, z)]
            f.append((b, b + 1, b + 2))
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def reference(name, n_views=1, h=H, w=W):
    """(vertices, faces, colors, cams, restatement outputs) of a named case; computed once, not to be modified."""
    if name in ("plane", "sphere", "wild"):
        v, f = {"plane": plane_mesh, "sphere": uv_sphere, "wild": wild_mesh}[name]()
        cams = view_cameras(n_views)
    else:
        v, f = {"clutter": clutter_mesh, "last_bit": last_bit_mesh}[name]()
        cams = pixel_camera()[None].repeat(n_views, 0)
    c = vertex_colors(len(v))
    return v, f, c, cams, render(v, f, cams, h, w, c)


# ---------------------------------------------------------------------------------------------------------------- analytic
def ray_sphere_depth(cam, centre_cam, radius, h, w):
    """z-depth of the pixel rays on a sphere around ``centre_cam`` (camera frame) -> (near depth, hit) [h,w]."""
    py, px = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rx, ry = _rays(cam, px.ravel(), py.ravel())
    r = np.stack([rx, ry, np.ones_like(rx)], 1)
    a, b = (r * r).sum(1), r @ centre_cam
    disc = b * b - a * (centre_cam @ centre_cam - radius * radius)
    hit = disc > 0
    lam = np.where(hit, (b - np.sqrt(np.where(hit, disc, 0.0))) / a, 0.0)
    return lam.reshape(h, w), hit.reshape(h, w)
