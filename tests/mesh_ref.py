"""A numpy restatement of the meshing rule of DESIGN §1.9 (include/cds_mvsnet_hip.h, "Sparse TSDF fusion and tetrahedra
extraction"): frame and allocation, integration, extraction.  fp64 where the rule says fp64, ``np.float32`` adds where it says
fp32.  It works on a dense copy of the lattice, which only small volumes allow; nothing here is shared with the kernels, and the
tetrahedron cases are not a table: every triangle is oriented by a geometric test on the tetrahedron's own corners.

A volume is a dict: origin float64 [3], voxel, trunc, nb int [3] (blocks per axis x, y, z), keys int64 [NB] ascending
(key = (bz nby + by) nbx + bx), sum float32 [NB,512], n / nc int32 [NB,512], rgb int32 [3,NB,512]; local index (lz 8 + ly) 8 + lx.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

MAX_CELLS = 1 << 26
KINDS = (1, 2, 4, 3, 5, 6, 7)          # edge kinds as corner offsets (bit 0: x, 1: y, 2: z): axes, face diagonals, body diagonal
PERMS = tuple(itertools.permutations(range(3)))      # the six axis orders, lexicographic


# ------------------------------------------------------------------------------------------------------ frame / allocation
def frame(points: np.ndarray, voxel: float):
    """origin [3] float64 and blocks per axis from the kept points [N,3] float32 (N >= 1)."""
    b = 8.0 * float(voxel)
    lo = points.min(0).astype(np.float64)
    hi = points.max(0).astype(np.float64)
    origin = (np.floor(lo / b) - 1.0) * b
    nb = np.floor((hi - origin) / b).astype(np.int64) + 2
    return origin, nb


def allocate(points: np.ndarray, voxel: float, trunc: float) -> dict:
    origin, nb = frame(points, voxel)
    assert int(nb[0]) * int(nb[1]) * int(nb[2]) <= MAX_CELLS
    bi = np.floor((points.astype(np.float64) - origin) / (8.0 * float(voxel))).astype(np.int64)
    own = np.unique(bi, axis=0)
    keys = set()
    for off in itertools.product((-1, 0, 1), repeat=3):
        c = own + np.array(off)
        ok = ((c >= 0) & (c < nb)).all(1)
        keys.update(((c[ok, 2] * nb[1] + c[ok, 1]) * nb[0] + c[ok, 0]).tolist())
    return empty_volume(origin, voxel, trunc, nb, np.array(sorted(keys), dtype=np.int64))


def empty_volume(origin, voxel, trunc, nb, keys) -> dict:
    k = len(keys)
    return {"origin": np.asarray(origin, np.float64), "voxel": float(voxel), "trunc": float(trunc), "nb": np.asarray(nb, np.int64),
            "keys": np.asarray(keys, np.int64), "sum": np.zeros((k, 512), np.float32), "n": np.zeros((k, 512), np.int32),
            "nc": np.zeros((k, 512), np.int32), "rgb": np.zeros((3, k, 512), np.int32)}


def lattice_index(vol: dict) -> np.ndarray:
    """Global lattice indices (x, y, z) of every stored point: int64 [NB,512,3]."""
    nb, keys = vol["nb"], vol["keys"]
    b = np.stack([keys % nb[0], (keys // nb[0]) % nb[1], keys // (nb[0] * nb[1])], 1)
    l = np.arange(512)
    loc = np.stack([l % 8, (l // 8) % 8, l // 64], 1)
    return 8 * b[:, None, :] + loc[None, :, :]


def lattice_points(vol: dict) -> np.ndarray:
    return vol["origin"] + lattice_index(vol).astype(np.float64) * vol["voxel"]


# ------------------------------------------------------------------------------------------------------------ integration
def integrate(vol: dict, depths: np.ndarray, masks: np.ndarray, images: np.ndarray, cams: np.ndarray) -> None:
    """depths [V,h,w] float32, masks [V,h,w] (non-zero: kept), images [V,h,w,3] uint8, cams [V,2,4,4] float32; in view order."""
    X = lattice_points(vol).reshape(-1, 3)
    T = vol["trunc"]
    s, n, nc = vol["sum"].reshape(-1), vol["n"].reshape(-1), vol["nc"].reshape(-1)
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
            sdf = d.astype(np.float64) - z
            ok &= ~(sdf < -T)
            tv = np.minimum(1.0, sdf / T).astype(np.float32)
            s[ok] = s[ok] + tv[ok]                       # float32 + float32
            n[ok] += 1
            near = ok & (sdf <= T)
            col = images[v][y, x].astype(np.int32)
            for c in range(3):
                rgb[c][near] += col[near, c]
            nc[near] += 1


# ------------------------------------------------------------------------------------------------------------- extraction
def _dense(vol: dict):
    nb = vol["nb"]
    shape = (8 * int(nb[2]), 8 * int(nb[1]), 8 * int(nb[0]))
    idx = lattice_index(vol)
    out = {"exists": np.zeros(shape, bool)}
    out["exists"][idx[..., 2], idx[..., 1], idx[..., 0]] = True
    for name in ("sum", "n", "nc"):
        a = np.zeros(shape, vol[name].dtype)
        a[idx[..., 2], idx[..., 1], idx[..., 0]] = vol[name]
        out[name] = a
    out["rgb"] = np.zeros((3,) + shape, np.int32)
    for c in range(3):
        out["rgb"][c][idx[..., 2], idx[..., 1], idx[..., 0]] = vol["rgb"][c]
    return out, shape


def _shift(a: np.ndarray, off: int, fill=False) -> np.ndarray:
    """b[L] = a[L + offset], ``fill`` where L + offset leaves the array; ``off``: corner bits, negative for L - offset."""
    sign = 1 if off >= 0 else -1
    off = abs(off)
    out = a
    for axis, bit in ((2, 1), (1, 2), (0, 4)):
        if off & bit:
            pad = np.full_like(out, fill)
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            src[axis] = slice(1, None) if sign > 0 else slice(None, -1)
            dst[axis] = slice(None, -1) if sign > 0 else slice(1, None)
            pad[tuple(dst)] = out[tuple(src)]
            out = pad
    return out


def _order_key(vol, z, y, x):
    nb = vol["nb"]
    return (((z // 8) * nb[1] + y // 8) * nb[0] + x // 8) * 512 + ((z % 8) * 8 + y % 8) * 8 + x % 8


def tet_corners(perm):
    """The corner offsets (bit masks) of the tetrahedron 000 -> +e_a -> +e_b -> 111 of axis order (a, b, c)."""
    a, b, _ = perm
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def _corner_xyz(o):
    return np.array([o & 1, (o >> 1) & 1, (o >> 2) & 1], np.float64)


def tet_triangles(perm, case):
    """The triangles of one tetrahedron for ``case`` (bit i: corner i is inside), as tuples of three edges (i, j), i < j, between
    tetrahedron corners.  One inside or one outside corner i with the others j < k < l: (ij, ik, il); two inside i < j and two
    outside k < l: the quadrilateral (ik, il, jl, jk) as (q0, q1, q2), (q0, q2, q3).  A triangle whose normal would point to the
    inside has its second and third vertex swapped; the test is made here on the edge midpoints of the real corners."""
    inside = [i for i in range(4) if case >> i & 1]
    outside = [i for i in range(4) if not case >> i & 1]
    if len(inside) in (0, 4):
        return []
    e = lambda i, j: (min(i, j), max(i, j))
    if len(inside) == 1 or len(outside) == 1:
        i = inside[0] if len(inside) == 1 else outside[0]
        j, k, l = [q for q in range(4) if q != i]
        tris = [[e(i, j), e(i, k), e(i, l)]]
    else:
        (i, j), (k, l) = inside, outside
        q = [e(i, k), e(i, l), e(j, l), e(j, k)]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    xyz = [_corner_xyz(o) for o in tet_corners(perm)]
    mid = lambda ed: 0.5 * (xyz[ed[0]] + xyz[ed[1]])
    towards = np.mean([xyz[i] for i in outside], 0) - np.mean([xyz[i] for i in inside], 0)
    a, b, c = (mid(ed) for ed in tris[0])
    if np.dot(np.cross(b - a, c - a), towards) < 0:
        tris = [[t[0], t[2], t[1]] for t in tris]
    return [tuple(t) for t in tris]


def extract(vol: dict, min_weight: int = 2) -> dict:
    """-> {"vertices" float32 [V,3], "colors" uint8 [V,3], "faces" int32 [F,3], "cubes" int64 [F,3]: the lattice index (x, y, z)
    of the cube each face came from}."""
    if len(vol["keys"]) == 0:
        return {"vertices": np.zeros((0, 3), np.float32), "colors": np.zeros((0, 3), np.uint8), "faces": np.zeros((0, 3), np.int32),
                "cubes": np.zeros((0, 3), np.int64)}
    d, shape = _dense(vol)
    valid = d["exists"] & (d["n"] >= int(min_weight))
    inside = d["sum"] < 0
    proc = np.ones(shape, bool)
    for o in range(8):
        proc &= _shift(valid, o)
    # vertices: (lower point, kind) whose edge changes sign and lies in a processed cube
    vid = np.full((7,) + shape, -1, np.int64)
    recs = []
    for kk, dmask in enumerate(KINDS):
        touched = np.zeros(shape, bool)
        for o in range(8):
            if o & dmask == 0:
                touched |= _shift(proc, -o)
        flag = touched & (inside != _shift(inside, dmask))
        z, y, x = np.nonzero(flag)
        recs.append(np.stack([_order_key(vol, z, y, x), np.full(z.shape, kk), z, y, x], 1))
    recs = np.concatenate(recs)
    recs = recs[np.lexsort((recs[:, 1], recs[:, 0]))]
    kk, z, y, x = recs[:, 1], recs[:, 2], recs[:, 3], recs[:, 4]
    vid[kk, z, y, x] = np.arange(len(recs))
    dm = np.array(KINDS)[kk]
    ia = np.stack([x, y, z], 1)
    ib = ia + np.stack([dm & 1, (dm >> 1) & 1, (dm >> 2) & 1], 1)
    za, ya, xa = ia[:, 2], ia[:, 1], ia[:, 0]
    zb, yb, xb = ib[:, 2], ib[:, 1], ib[:, 0]
    Da = d["sum"][za, ya, xa].astype(np.float64) / d["n"][za, ya, xa]
    Db = d["sum"][zb, yb, xb].astype(np.float64) / d["n"][zb, yb, xb]
    tt = Da / (Da - Db)
    Xa = vol["origin"] + ia.astype(np.float64) * vol["voxel"]
    Xb = vol["origin"] + ib.astype(np.float64) * vol["voxel"]
    verts = (Xa + tt[:, None] * (Xb - Xa)).astype(np.float32)
    nca, ncb = d["nc"][za, ya, xa].astype(np.int64), d["nc"][zb, yb, xb].astype(np.int64)
    cols = np.zeros((len(recs), 3), np.uint8)
    for c in range(3):
        ca = (2 * d["rgb"][c][za, ya, xa].astype(np.int64) + nca) // np.maximum(2 * nca, 1)
        cb = (2 * d["rgb"][c][zb, yb, xb].astype(np.int64) + ncb) // np.maximum(2 * ncb, 1)
        ca = np.where(nca > 0, ca, cb)
        cb = np.where(ncb > 0, cb, ca)
        val = np.floor((ca.astype(np.float64) + tt * (cb - ca).astype(np.float64)) + 0.5)
        val = np.where((nca == 0) & (ncb == 0), 128.0, val)
        cols[:, c] = np.clip(val, 0, 255).astype(np.uint8)
    # faces
    z, y, x = np.nonzero(proc)
    ckey = _order_key(vol, z, y, x)
    ins = [_shift(inside, o)[z, y, x] for o in range(8)]
    faces, keys, cubes = [], [], []
    for t, perm in enumerate(PERMS):
        corners = tet_corners(perm)
        case = sum(ins[corners[i]].astype(np.int64) << i for i in range(4))
        for cs in range(1, 15):
            sel = np.nonzero(case == cs)[0]
            if sel.size == 0:
                continue
            for ti, tri in enumerate(tet_triangles(perm, cs)):
                ids = []
                for (i, j) in tri:
                    oi, oj = corners[i], corners[j]
                    kk = KINDS.index(oi ^ oj)
                    ids.append(vid[kk, z[sel] + ((oi >> 2) & 1), y[sel] + ((oi >> 1) & 1), x[sel] + (oi & 1)])
                faces.append(np.stack(ids, 1))
                keys.append(np.stack([ckey[sel], np.full(sel.shape, t), np.full(sel.shape, ti)], 1))
                cubes.append(np.stack([x[sel], y[sel], z[sel]], 1))
    if not faces:
        return {"vertices": verts, "colors": cols, "faces": np.zeros((0, 3), np.int32), "cubes": np.zeros((0, 3), np.int64)}
    faces, keys, cubes = np.concatenate(faces), np.concatenate(keys), np.concatenate(cubes)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    assert (faces >= 0).all()
    return {"vertices": verts, "colors": cols, "faces": faces[order].astype(np.int32), "cubes": cubes[order]}


# ------------------------------------------------------------------------------------------------------------ measurements
def topology(faces: np.ndarray, n_vertices: int) -> dict:
    """Edge statistics of a triangle list: use counts of undirected edges, whether every directed edge is unique and has its
    reverse, Euler characteristic V - E + F over the vertices that faces use."""
    f = faces.astype(np.int64)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    code = de[:, 0] * n_vertices + de[:, 1]
    rev = de[:, 1] * n_vertices + de[:, 0]
    und = np.minimum(de[:, 0], de[:, 1]) * n_vertices + np.maximum(de[:, 0], de[:, 1])
    _, counts = np.unique(und, return_counts=True)
    ucode = np.unique(code)
    return {"edge_uses": counts, "edges": len(counts), "directed_unique": len(ucode) == len(code),
            "reverse_present": bool(np.isin(rev, ucode).all()), "used_vertices": len(np.unique(f)),
            "euler": len(np.unique(f)) - len(counts) + len(f)}


def signed_volume(vertices: np.ndarray, faces: np.ndarray) -> float:
    v = vertices.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def degenerate_faces(vertices: np.ndarray, faces: np.ndarray) -> int:
    v = vertices.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return int((np.linalg.norm(np.cross(b - a, c - a), axis=1) == 0).sum())


# ----------------------------------------------------------------------------------------------------------------- scenes
def analytic_volume(centre, radius, blocks=3, voxel=1.0, drop=None) -> dict:
    """|X - c| - r on a (8 blocks)^3 lattice with origin 0, stored as accumulators: n = 2, sum = float32(2 * clamp(sdf / T, -1, 1))
    with T = 4 voxels; colours from the lattice index.  ``drop``: a block (bx, by, bz) left out."""
    nb = np.array([blocks] * 3, np.int64)
    keys = [k for k in range(blocks ** 3)
            if drop is None or (k % blocks, (k // blocks) % blocks, k // blocks ** 2) != tuple(drop)]
    vol = empty_volume(np.zeros(3), voxel, 4.0 * voxel, nb, keys)
    idx = lattice_index(vol)
    X = lattice_points(vol)
    sdf = np.linalg.norm(X - np.asarray(centre, np.float64), axis=-1) - radius
    vol["sum"][:] = (2.0 * np.clip(sdf / vol["trunc"], -1.0, 1.0)).astype(np.float32)
    vol["n"][:] = 2
    vol["nc"][:] = np.where(idx.sum(-1) % 5 == 0, 0, 2)            # some points without a colour
    for c in range(3):
        vol["rgb"][c] = np.where(vol["nc"] > 0, 2 * ((idx[..., c] * (9 + 2 * c) + 40 * c) % 256) + (idx[..., (c + 1) % 3] % 2), 0)
    return vol


def sphere_scene(radius_vox=9.0, voxel=0.5, size=48, centre=(3.1, -2.3, 40.7)):
    """26 cameras on the directions {-1,0,1}^3 \\ 0 at 4 r from a sphere of r = radius_vox voxels, looking at its centre;
    analytic z-depth maps through the pixel centres.  -> depths, masks, images, cams, points (the kept world points), centre, r."""
    r = radius_vox * voxel
    c = np.asarray(centre, np.float64)
    f = 0.5 * size / np.tan(np.arcsin(0.25) * 1.35)                # the sphere fills about three quarters of the map
    K = np.array([[f, 0, size / 2], [0, f, size / 2], [0, 0, 1]], np.float64)
    depths, masks, images, cams, points = [], [], [], [], []
    ys, xs = np.meshgrid(np.arange(size) + 0.5, np.arange(size) + 0.5, indexing="ij")
    rays = np.linalg.inv(K) @ np.stack([xs, ys, np.ones_like(xs)], 0).reshape(3, -1)           # camera frame, z = 1
    for n, dr in enumerate(d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)):
        dr = np.asarray(dr, np.float64) / np.linalg.norm(dr)
        eye = c + 4.0 * r * dr
        fwd = -dr
        up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
        right = np.cross(up, fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])                             # world -> camera
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = R, -R @ eye
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3], cam[1, 3, 3] = E, K, 1.0
        # ray / sphere in the camera frame: centre at (0, 0, 4 r)
        cc = np.array([0.0, 0.0, 4.0 * r])
        a = (rays * rays).sum(0)
        b = rays.T @ cc
        disc = b * b - a * (cc @ cc - r * r)
        hit = disc > 0
        lam = np.where(hit, (b - np.sqrt(np.where(hit, disc, 0))) / a, 0.0)          # z-depth: the rays have z = 1
        depth = lam.reshape(size, size).astype(np.float32)
        mask = hit.reshape(size, size)
        P = (R.T @ (rays * lam) + eye[:, None]).T                  # world points of the pixels: R^T (Xc - t), t = -R eye
        points.append(P[hit].astype(np.float32))
        img = np.zeros((size, size, 3), np.uint8)
        img[..., 0] = (np.arange(size)[None, :] * 5 + 3 * n) % 256
        img[..., 1] = (np.arange(size)[:, None] * 4 + 7 * n) % 256
        img[..., 2] = (40 + 8 * n) % 256
        depths.append(depth), masks.append(mask.astype(np.uint8)), images.append(img), cams.append(cam)
    return {"depths": np.stack(depths), "masks": np.stack(masks), "images": np.stack(images), "cams": np.stack(cams),
            "points": np.concatenate(points), "centre": c, "radius": r, "voxel": voxel}


ANALYTIC = {"sphere": dict(centre=(9.3, 9.7, 9.1), radius=6.37), "aligned": dict(centre=(9.0, 10.0, 9.0), radius=6.0),
            "hole": dict(centre=(9.3, 9.7, 9.1), radius=6.37, drop=(1, 1, 0))}


@functools.lru_cache(maxsize=None)
def analytic_case(name: str):
    """(volume, its mesh at min_weight 2) of the three analytic volumes; computed once, not to be modified."""
    vol = analytic_volume(**ANALYTIC[name])
    return vol, extract(vol, 2)


@functools.lru_cache(maxsize=None)
def sphere_case():
    """(scene, integrated volume, mesh) of :func:`sphere_scene` with T = 2.5 voxels and min_weight 2; computed once."""
    sc = sphere_scene()
    vol = allocate(sc["points"], sc["voxel"], 2.5 * sc["voxel"])
    integrate(vol, sc["depths"], sc["masks"], sc["images"], sc["cams"])
    return sc, vol, extract(vol, 2)


def integration_scene(n_views: int, h: int = 37, w: int = 50, voxel: float = 0.25, seed: int = 0):
    """Views of the plane z = 0 for the integration tests; the maps need not agree with each other, they need every case of
    the rule.  Kept points: a jittered 4 x 4 patch of the plane (2 x 2 blocks of side 2 and their neighbours: the allocated
    blocks reach the border of the block grid on every side).  Cameras: in front of the plane at z = -9..-5, looking at the
    patch with a narrow field of view, so that part of the lattice projects outside the map; every third view sits inside the
    volume and looks along the plane, so that part of the lattice is behind it.  Depth: the ray's z-depth to the plane plus a
    ripple of +-0.6 (sdf on either side of +-T for T between 1 and 8 voxels), then pixels set to 0, NaN, +inf, -inf and a negative
    number, and a mask that drops one pixel in eight.  -> depths, masks, images, cams, points."""
    rs = np.random.RandomState(100 + seed)
    g = np.arange(-2.0, 2.0, 0.05) + 0.02
    px, py = np.meshgrid(g, g, indexing="ij")
    points = np.stack([px.ravel(), py.ravel(), rs.uniform(-0.05, 0.05, px.size)], 1).astype(np.float32)
    f = 1.6 * w
    K = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1]], np.float64)
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    rays = np.linalg.inv(K) @ np.stack([xs, ys, np.ones_like(xs)], 0).reshape(3, -1)
    depths, masks, images, cams = [], [], [], []
    for v in range(n_views):
        if v % 3 == 2:
            eye = np.array([rs.uniform(-1, 1), rs.uniform(-1, 1), rs.uniform(-0.6, -0.2)])
            target = eye + np.array([np.cos(v), np.sin(v), 0.25])
        else:
            eye = np.array([rs.uniform(-3, 3), rs.uniform(-3, 3), rs.uniform(-9, -5)])
            target = np.array([rs.uniform(-1.5, 1.5), rs.uniform(-1.5, 1.5), 0.0])
        fwd = (target - eye) / np.linalg.norm(target - eye)
        right = np.cross(np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([1.0, 0.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0, :3, :3], cam[0, :3, 3], cam[0, 3, 3] = R, -R @ eye, 1.0
        cam[1, :3, :3], cam[1, 3, 3] = K, 1.0
        wz = (R.T @ rays)[2]
        lam = np.where(wz > 1e-6, -eye[2] / np.where(wz > 1e-6, wz, 1.0), 0.0)              # z-depth of the plane along the ray
        lam = np.where((lam > 0) & (lam < 30), lam + 0.6 * np.sin(3.0 * xs.ravel() / w * np.pi + v) * np.cos(0.4 * ys.ravel()), 0.0)
        depth = lam.reshape(h, w).astype(np.float32)
        for k, bad in enumerate((0.0, np.nan, np.inf, -np.inf, -3.0)):
            depth[rs.randint(0, h, 6), rs.randint(0, w, 6)] = bad
        depths.append(depth)
        masks.append((rs.rand(h, w) > 0.125).astype(np.uint8))
        images.append(rs.randint(0, 256, (h, w, 3)).astype(np.uint8))
        cams.append(cam)
    return {"depths": np.stack(depths), "masks": np.stack(masks), "images": np.stack(images), "cams": np.stack(cams),
            "points": points, "voxel": voxel}


@functools.lru_cache(maxsize=None)
def integration_case(n_views: int, trunc_voxels: float):
    """(scene, integrated volume) of :func:`integration_scene`; computed once, not to be modified."""
    sc = integration_scene(n_views)
    vol = allocate(sc["points"], sc["voxel"], trunc_voxels * sc["voxel"])
    integrate(vol, sc["depths"], sc["masks"], sc["images"], sc["cams"])
    return sc, vol
