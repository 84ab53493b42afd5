"""A numpy restatement of the simplification rule of DESIGN §1.12 (include/cds_mvsnet_hip.h, "Simplification of a triangle mesh:
vertex clustering with quadric placement"), and the meshes the tests of csrc/mesh_simplify.hip share.  Plain loops where the rule
fixes an order: Python floats are IEEE doubles and Python never contracts a product and a sum.  No kernel, no torch."""
import functools

import numpy as np


# ------------------------------------------------------------------------------------------------------------------ the rule
def cell_keys(vertices: np.ndarray, cell: float) -> np.ndarray:
    """Rule 1: origin o = float32(min - cell / 2); index floorf((p - o) / cell) per axis in fp32; the 63-bit key puts the index >> 3
    of x, y, z (18 bits each) above the low three bits of x, y, z."""
    p = np.asarray(vertices, np.float32)
    h = np.float32(cell)
    o = (p.min(0).astype(np.float64) - 0.5 * float(cell)).astype(np.float32)
    c = np.maximum(np.floor((p - o[None, :]) / h).astype(np.int64), 0)
    coarse = ((c[:, 0] >> 3) << 36) | ((c[:, 1] >> 3) << 18) | (c[:, 2] >> 3)
    local = ((c[:, 0] & 7) << 6) | ((c[:, 1] & 7) << 3) | (c[:, 2] & 7)
    return (coarse << 9) | local


def clusters(vertices: np.ndarray, cell: float):
    """Rule 1 -> (cluster int64 [V]: the rank of each vertex's key among the occupied keys, C)."""
    ukeys, cluster = np.unique(cell_keys(vertices, cell), return_inverse=True)
    return cluster.reshape(-1).astype(np.int64), len(ukeys)


def means(vertices, colors, cluster, n_clusters):
    """Rule 2 -> (m float64 [C,3], colour uint8 [C,3], k int64 [C]); the members of a cluster in ascending vertex index."""
    s = np.zeros((n_clusters, 3), np.float64)
    cs = np.zeros((n_clusters, 3), np.int64)
    k = np.zeros(n_clusters, np.int64)
    p = np.asarray(vertices, np.float32).astype(np.float64)
    for v in range(len(p)):                                              # ascending v: sequential per cluster
        c = cluster[v]
        s[c] += p[v]
        cs[c] += colors[v].astype(np.int64)
        k[c] += 1
    return s / k[:, None], ((2 * cs + k[:, None]) // (2 * k[:, None])).astype(np.uint8), k


def quadric_positions(vertices, faces, cluster, m, cell):
    """Rules 3 and 4 -> (positions float32 [C,3], fallback bool [C])."""
    nc = len(m)
    p = np.asarray(vertices, np.float32).astype(np.float64)
    A = [[0.0] * 6 for _ in range(nc)]                                   # A00 A01 A02 A11 A12 A22
    B = [[0.0] * 3 for _ in range(nc)]
    mm = m.tolist()
    inf = float("inf")
    for f, tri in enumerate(np.asarray(faces, np.int64).tolist()):       # ascending (f, j): sequential per cluster
        p0, p1, p2 = (p[i].tolist() for i in tri)
        e1 = [p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]]
        e2 = [p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]]
        nx, ny, nz = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
        w2 = (nx * nx + ny * ny) + nz * nz
        if not (0.0 < w2 < inf):
            continue
        for j in range(3):
            c = cluster[tri[j]]
            q = [p0[0] - mm[c][0], p0[1] - mm[c][1], p0[2] - mm[c][2]]
            d = (nx * q[0] + ny * q[1]) + nz * q[2]
            a, b = A[c], B[c]
            a[0] += nx * nx; a[1] += nx * ny; a[2] += nx * nz; a[3] += ny * ny; a[4] += ny * nz; a[5] += nz * nz
            b[0] += nx * d; b[1] += ny * d; b[2] += nz * d
    pos = np.empty((nc, 3), np.float32)
    fallback = np.zeros(nc, bool)
    lim = float(np.float32(cell))
    with np.errstate(all="ignore"):
        for c in range(nc):
            a00, a01, a02, a11, a12, a22 = (np.float64(x) for x in A[c])
            b0, b1, b2 = (np.float64(x) for x in B[c])
            tr = (a00 + a11) + a22
            lam = tr * np.float64(2.0 ** -10)
            m00, m11, m22 = a00 + lam, a11 + lam, a22 + lam
            c00, c01, c02 = m11 * m22 - a12 * a12, a02 * a12 - a01 * m22, a01 * a12 - a02 * m11
            c11, c12, c22 = m00 * m22 - a02 * a02, a01 * a02 - m00 * a12, m00 * m11 - a01 * a01
            det = (m00 * c00 + a01 * c01) + a02 * c02
            y = np.array([((c00 * b0 + c01 * b1) + c02 * b2) / det, ((c01 * b0 + c11 * b1) + c12 * b2) / det,
                          ((c02 * b0 + c12 * b1) + c22 * b2) / det], np.float64)
            ok = np.isfinite(tr) and tr > 0 and np.isfinite(det) and det > 0 and np.isfinite(y).all() and np.abs(y).max() <= lim
            fallback[c] = not ok
            pos[c] = (m[c] + y).astype(np.float32) if ok else m[c].astype(np.float32)
    return pos, fallback


def simplify(vertices, colors, faces, cell, placement="quadric"):
    """Rules 1-6 -> ({"vertices", "colors", "faces"}, info as mesh.simplify_mesh's, detail: {"cluster" [V], "positions" [C,3],
    "colors" [C,3], "fallback" bool [C], "kept" bool [C], "face_keep" bool [F], "collapsed" bool [F], "incidences" int64 [C]})."""
    vertices, colors = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(colors, np.uint8).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nv, nf = len(vertices), len(faces)
    if nv == 0 or nf == 0:
        out = {"vertices": np.zeros((0, 3), np.float32), "colors": np.zeros((0, 3), np.uint8), "faces": np.zeros((0, 3), np.int32)}
        return out, {"vertices": (nv, 0), "faces": (0, 0), "clusters": 0, "collapsed": 0, "duplicates": 0, "fallback": 0}, None
    cluster, nc = clusters(vertices, cell)
    m, col, _ = means(vertices, colors, cluster, nc)
    if placement == "quadric":
        pos, fallback = quadric_positions(vertices, faces, cluster, m, cell)
    elif placement == "mean":
        pos, fallback = m.astype(np.float32), np.zeros(nc, bool)
    else:
        raise ValueError(placement)
    fc = cluster[faces]                                                  # rule 5
    collapsed = (fc[:, 0] == fc[:, 1]) | (fc[:, 1] == fc[:, 2]) | (fc[:, 0] == fc[:, 2])
    seen, fkeep = set(), np.zeros(nf, bool)
    for f in range(nf):
        if collapsed[f]:
            continue
        t = fc[f].tolist()
        r = t.index(min(t))
        ident = (t[r], t[(r + 1) % 3], t[(r + 2) % 3])
        if ident not in seen:
            seen.add(ident)
            fkeep[f] = True
    kept = np.zeros(nc, bool)                                            # rule 6
    kept[fc[fkeep].reshape(-1)] = True
    new = np.cumsum(kept) - 1
    out = {"vertices": pos[kept], "colors": col[kept], "faces": new[fc[fkeep]].astype(np.int32).reshape(-1, 3)}
    info = {"vertices": (nv, int(kept.sum())), "faces": (nf, int(fkeep.sum())), "clusters": nc, "collapsed": int(collapsed.sum()),
            "duplicates": int(nf - collapsed.sum() - fkeep.sum()), "fallback": int(fallback.sum())}
    detail = {"cluster": cluster, "positions": pos, "colors": col, "fallback": fallback, "kept": kept, "face_keep": fkeep,
              "collapsed": collapsed, "incidences": np.bincount(fc.reshape(-1), minlength=nc)}
    return out, info, detail


# ------------------------------------------------------------------------------------------------------------ measurements
def closed(faces: np.ndarray) -> bool:
    """Every directed edge has its reverse among the directed edges."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return True
    n = int(f.max()) + 1
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return bool(np.isin(de[:, 1] * n + de[:, 0], de[:, 0] * n + de[:, 1]).all())


def ulp_distance(a: np.ndarray, b: np.ndarray) -> int:
    """The largest distance, in representable fp32 values, between two float32 arrays of finite numbers."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return int(np.abs(ordered(a) - ordered(b)).max()) if a.size else 0


# ---------------------------------------------------------------------------------------------------------------- meshes
def colors_for(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def _weld(points: np.ndarray, quads):
    """Quads over float64 points with repeats -> (float32 vertices welded by rounded position, triangles: two per quad)."""
    key = np.round(points * 4096).astype(np.int64)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    tris = []
    for a, b, c, d in quads:
        tris += [[inverse[a], inverse[b], inverse[c]], [inverse[a], inverse[c], inverse[d]]]
    return points[first].astype(np.float32), np.array(tris, np.int32)


@functools.lru_cache(maxsize=None)
def cube(side: float = 4.0, n: int = 16, offset=(0.13, -0.21, 0.37)):
    """The surface of [0, side]^3 + offset: n x n quads per side, two triangles each, welded, outward winding:
    6 n^2 + 2 vertices and 12 n^2 faces.  -> (vertices, colors, faces); computed once, not to be modified."""
    t = np.linspace(0.0, side, n + 1)
    pts, quads = [], []
    for axis in range(3):
        for hi in (0, 1):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            base = len(pts)
            for i in range(n + 1):
                for j in range(n + 1):
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[u], p[v] = side * hi, t[i], t[j]
                    pts.append(p)
            for i in range(n):
                for j in range(n):
                    a, b = base + i * (n + 1) + j, base + (i + 1) * (n + 1) + j
                    q = (a, b, b + 1, a + 1)                             # u x v = +axis: outward on the high side
                    quads.append(q if hi else q[::-1])
    v, f = _weld(np.array(pts, np.float64), quads)
    v = (v.astype(np.float64) + np.asarray(offset, np.float64)).astype(np.float32)
    return v, colors_for(len(v), 11), f


def cube_errors(vertices: np.ndarray, side: float = 4.0, offset=(0.13, -0.21, 0.37)):
    """-> (the largest distance from a cube corner to its nearest vertex, the largest distance of a vertex from the cube's
    surface), for vertices inside or on the cube up to rounding."""
    p = vertices.astype(np.float64) - np.asarray(offset, np.float64)
    corners = np.array([[x, y, z] for x in (0, side) for y in (0, side) for z in (0, side)], np.float64)
    corner = max(float(np.linalg.norm(p - c, axis=1).min()) for c in corners)
    outside = np.linalg.norm(np.maximum(np.maximum(-p, p - side), 0.0), axis=1)
    inside = np.minimum(p, side - p).min(1)
    return corner, float(np.where(outside > 0, outside, np.abs(inside)).max())


def tilted_plane(n: int = 24, depth: float = 650.0, seed: int = 5):
    """An n x n grid of quads (spacing 0.37) on the plane through (0, 0, depth) with normal (0.3, -0.2, 1) / |.|, each vertex the
    fp32 rounding of a point of the plane.  -> (vertices, colors, faces, unit normal float64, a point of the plane)."""
    nrm = np.array([0.3, -0.2, 1.0])
    nrm /= np.linalg.norm(nrm)
    u = np.cross(nrm, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    w = np.cross(nrm, u)
    origin = np.array([0.0, 0.0, depth])
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    pts = origin + 0.37 * (i.reshape(-1, 1) * u + j.reshape(-1, 1) * w)
    quads = [(a, a + n + 1, a + n + 2, a + 1) for a in (ii * (n + 1) + jj for ii in range(n) for jj in range(n))]
    tris = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return pts.astype(np.float32), colors_for(len(pts), seed), tris, nrm, origin


def plate(n: int = 12, gap: float = 0.05):
    """Two n x n sheets of quads (spacing 0.4) at z = 0.3 and z = 0.3 + gap with opposite windings, not connected: a thin plate
    without its rim.  -> (vertices, colors, faces)."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    xy = np.stack([0.11 + 0.4 * i.reshape(-1), -0.07 + 0.4 * j.reshape(-1)], 1)
    lo = np.concatenate([xy, np.full((len(xy), 1), 0.3)], 1)
    hi = np.concatenate([xy, np.full((len(xy), 1), 0.3 + gap)], 1)
    quads = [(a, a + n + 1, a + n + 2, a + 1) for a in (ii * (n + 1) + jj for ii in range(n) for jj in range(n))]
    up = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    v = np.concatenate([lo, hi]).astype(np.float32)
    return v, colors_for(len(v), 6), np.concatenate([up[:, ::-1], up + len(xy)]).astype(np.int32)


def cone_band(apex_cells: float, slope: float, cell: float = 1.0, n: int = 12):
    """A band of a cone (axis z, radius = slope x height above the apex; two rings of n vertices at heights (apex_cells -+ 0.04)
    cell, 2 n triangles) inside the cell around (10, 10, 10) cell, and one long face that ties the band's vertex 0 to two
    vertices near the origin, 10^-3 cell apart along the cone's generator through vertex 0: the face fixes the frame (the minimum
    is the origin, so cells run from k - 1/2 to k + 1/2), lies in a plane through the apex like every tangent plane of the
    cone, and has about the squared area of a few band faces.  -> (vertices, colors, faces, apex float64 [3], the band's
    vertex indices)."""
    mid = np.array([10.02, 9.97, 10.0]) * cell
    apex = mid - np.array([0.0, 0.0, apex_cells * cell])
    ang = 2 * np.pi * np.arange(n) / n
    rings = []
    for h in ((apex_cells - 0.04) * cell, (apex_cells + 0.04) * cell):
        rings.append(apex + np.stack([slope * h * np.cos(ang), slope * h * np.sin(ang), np.full(n, h)], 1))
    band = np.concatenate(rings)
    g = band[0] - apex
    far = np.array([[0.0, 0.0, 0.0], 1e-3 * cell * g / np.linalg.norm(g)])
    v = np.concatenate([band, far]).astype(np.float32)
    tris = []
    for k in range(n):
        a, b = k, (k + 1) % n
        tris += [[a, b, n + b], [a, n + b, n + a]]
    tris.append([0, 2 * n, 2 * n + 1])
    return v, colors_for(len(v), 8), np.array(tris, np.int32), apex, np.arange(2 * n)


def fan_and_triangles(n_fan: int = 3000, n_small: int = 400, seed: int = 3):
    """A fan of n_fan triangles around one vertex, the whole fan inside one cell of side 1 (one cluster with 3 n_fan incidences,
    every face of it collapsed), next to n_small small triangles spread over many cells, interleaved in face order.
    -> (vertices, colors, faces)."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n_fan + 1) / (n_fan + 1)
    rim = np.stack([50.5 + 0.3 * np.cos(ang), 50.5 + 0.3 * np.sin(ang), 50.5 + 0.1 * np.sin(3 * ang)], 1)
    hub = np.array([[50.5, 50.5, 50.6]])
    fan = np.stack([np.zeros(n_fan, np.int64), 1 + np.arange(n_fan), 2 + np.arange(n_fan)], 1)
    base = rng.uniform(40.0, 60.0, (n_small, 1, 3))
    small = base + rng.uniform(-1.5, 1.5, (n_small, 3, 3))
    v = np.concatenate([hub, rim, small.reshape(-1, 3)]).astype(np.float32)
    tri = (n_fan + 2 + np.arange(3 * n_small)).reshape(n_small, 3)
    faces = np.insert(fan, np.arange(n_small) * (n_fan // n_small), tri, axis=0)
    return v, colors_for(len(v), seed), np.ascontiguousarray(faces, np.int32)
