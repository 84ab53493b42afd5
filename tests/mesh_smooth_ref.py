"""A numpy restatement of the smoothing rule of DESIGN §1.15 (include/cds_mvsnet_hip.h, "Smoothing of a triangle mesh"), and the
meshes the tests of csrc/mesh_smooth.hip share.  Sorted arrays and slot-wise fp64 sums; no kernel, no torch."""
import functools

import numpy as np

import mesh_clean_ref as C
import mesh_ref as M

TAIL = 64                              # neighbours summed slot by slot over all vertices; a longer list is finished on its own


def adjacency(faces: np.ndarray, n_vertices: int) -> dict:
    """Rules 1-3 -> {"start" int32 [V+1], "degree" int32 [V], "neighbors" int32 [E] (the slack of a segment is -1), "boundary",
    "isolated" bool [V]}: the layout of mesh.mesh_adjacency."""
    nv = int(n_vertices)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[((f >= 0) & (f < nv)).all(1)]
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)                     # the slots (0,1), (1,2), (2,0)
    keep = a != b
    i, j = np.concatenate([a[keep], b[keep]]), np.concatenate([b[keep], a[keep]])       # an entry at either end of a slot
    count = np.bincount(i, minlength=nv).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(count)])
    pairs, mult = np.unique(i * max(nv, 1) + j, return_counts=True)         # ascending (i, j); the multiplicity of {i,j}
    ui, uj = pairs // max(nv, 1), pairs % max(nv, 1)
    boundary = np.zeros(nv, bool)
    boundary[ui[mult == 1]] = True
    sel = ~boundary[ui] | (mult == 1)                                     # rule 3
    ui, uj = ui[sel], uj[sel]
    deg = np.bincount(ui, minlength=nv).astype(np.int64)
    nbr = np.full(int(start[-1]), -1, np.int32)
    first = np.concatenate([[0], np.cumsum(deg)])[:-1]
    nbr[start[ui] + (np.arange(len(ui)) - first[ui])] = uj
    return {"start": start.astype(np.int32), "degree": deg.astype(np.int32), "neighbors": nbr, "boundary": boundary,
            "isolated": deg == 0}


def used(adj: dict) -> np.ndarray:
    """The neighbours of every vertex one after the other, without the slack."""
    start, deg = adj["start"].astype(np.int64), adj["degree"].astype(np.int64)
    owner = np.repeat(np.arange(len(deg)), deg)
    first = np.concatenate([[0], np.cumsum(deg)])[:-1]
    return adj["neighbors"][start[owner] + (np.arange(len(owner)) - first[owner])]


def step(p: np.ndarray, adj: dict, s: float) -> np.ndarray:
    """Rule 4: float32 [V,3] -> float32 [V,3]."""
    start, deg, nbr = adj["start"].astype(np.int64)[:-1], adj["degree"].astype(np.int64), adj["neighbors"]
    acc = np.zeros((len(p), 3), np.float64)
    for k in range(int(min(deg.max(initial=0), TAIL))):                  # slot k of every vertex that has one: ascending j
        has = deg > k
        acc[has] += p[nbr[start[has] + k]]
    for v in np.nonzero(deg > TAIL)[0]:                                  # a hub: the rest of its list, still in order
        rest = p[nbr[start[v] + TAIL:start[v] + deg[v]]].astype(np.float64)
        acc[v] = np.cumsum(np.concatenate([acc[v][None], rest]), axis=0)[-1]          # cumsum adds sequentially
    out = p.copy()
    has = deg > 0
    p64 = p[has].astype(np.float64)
    m = acc[has] / deg[has, None].astype(np.float64)
    out[has] = (p64 + s * (m - p64)).astype(np.float32)
    return out


def limit(p0: np.ndarray, p: np.ndarray, max_move: float):
    """Rules 6 and 8 -> (positions, n2 float64 [V] before the clamp, clamped bool [V])."""
    o = p0.astype(np.float64)
    d = p.astype(np.float64) - o
    n2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    D = float(max_move)
    clamped = (n2 > D * D) if D > 0 else np.zeros(len(p), bool)
    out = p.copy()
    if clamped.any():
        scale = D / np.sqrt(n2[clamped])
        out[clamped] = (o[clamped] + d[clamped] * scale[:, None]).astype(np.float32)
    return out, n2, clamped


def smooth(vertices, colors, faces, iterations, lam=0.5, mu=-0.53, max_move=0.0, adj=None):
    """Rules 1-8 -> ({"vertices", "colors", "faces"}, info as mesh.smooth_mesh's)."""
    p0 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nv = len(p0)
    info = {"iterations": int(iterations), "lam": float(lam), "mu": float(mu), "vertices": nv, "boundary": 0, "isolated": nv,
            "clamped": 0, "max_move": 0.0}
    out = {"vertices": p0, "colors": colors, "faces": faces}
    adj = adjacency(faces, nv) if adj is None else adj
    if nv == 0 or len(adj["neighbors"]) == 0:                            # no valid edge
        return out, info
    p = p0
    for _ in range(int(iterations)):
        p = step(p, adj, float(lam))
        if mu != 0:
            p = step(p, adj, float(mu))
    p, n2, clamped = limit(p0, p, max_move)
    info.update(boundary=int(adj["boundary"].sum()), isolated=int(adj["isolated"].sum()), clamped=int(clamped.sum()),
                max_move=float(np.sqrt(n2.max())))
    return dict(out, vertices=p), info


# ---------------------------------------------------------------------------------------------------------------- meshes
SPHERE = M.ANALYTIC["sphere"]


def sphere():
    m = M.analytic_case("sphere")[1]
    return m["vertices"], m["colors"], m["faces"]


@functools.lru_cache(maxsize=None)
def noisy_sphere(sigma: float = 0.1, seed: int = 0):
    """The analytic sphere with normal noise of ``sigma`` voxels along the radius; computed once, not to be modified."""
    v, c, f = sphere()
    centre = np.asarray(SPHERE["centre"], np.float64)
    r = v.astype(np.float64) - centre
    unit = r / np.linalg.norm(r, axis=1, keepdims=True)
    noise = np.random.default_rng(seed).normal(0, sigma, (len(v), 1))
    return (v.astype(np.float64) + noise * unit).astype(np.float32), c, f


def sphere_errors(vertices, faces):
    """-> (rms radial error, mean angle in degrees between the face normals and the radii through the face centres)."""
    centre = np.asarray(SPHERE["centre"], np.float64)
    v = vertices.astype(np.float64)
    rms = float(np.sqrt(np.mean((np.linalg.norm(v - centre, axis=1) - SPHERE["radius"]) ** 2)))
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = np.cross(b - a, c - a)
    rad = (a + b + c) / 3.0 - centre
    cos = np.abs((n * rad).sum(1)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(rad, axis=1))
    return rms, float(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))).mean())


def grid_patch(nx: int = 9, ny: int = 7, seed: int = 1, z: float = 2.5, jitter: float = 0.3):
    """An open nx x ny patch in the plane z, the vertices jittered inside the plane (the border ones along their line, the
    corners not at all), two triangles per cell
    -> (vertices, colors, faces)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    jit = rng.uniform(-1.0, 1.0, (ny, nx, 2)) * jitter
    v = np.stack([xs + jit[..., 0], ys + jit[..., 1], np.full_like(xs, z)], -1)
    v[0, :, 1], v[-1, :, 1], v[:, 0, 0], v[:, -1, 0] = 0.0, ny - 1.0, 0.0, nx - 1.0      # the border stays on its four lines
    v[0, 0, :2], v[0, -1, :2], v[-1, 0, :2], v[-1, -1, :2] = (0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)
    idx = np.arange(nx * ny).reshape(ny, nx)
    q = np.stack([idx[:-1, :-1], idx[:-1, 1:], idx[1:, 1:], idx[1:, :-1]], -1).reshape(-1, 4)
    f = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]]).astype(np.int32)
    return v.reshape(-1, 3).astype(np.float32), C._colors(nx * ny, seed), f


def hub_fan(valence: int = 5000, seed: int = 2):
    """A closed fan: the hub 0 and a ring of ``valence`` vertices, every ring edge also in a face with an outer vertex, so the hub
    is interior with that many neighbours -> (vertices, colors, faces)."""
    n = int(valence)
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(ang), np.sin(ang), 0.05 * rng.normal(size=n)], 1) * 50.0
    outer = np.stack([1.1 * np.cos(ang + np.pi / n), 1.1 * np.sin(ang + np.pi / n), 0.05 * rng.normal(size=n)], 1) * 50.0
    v = np.concatenate([[[0.3, -0.2, 4.0]], ring, outer]).astype(np.float32)
    r = 1 + np.arange(n)
    nxt = 1 + (np.arange(n) + 1) % n
    f = np.concatenate([np.stack([np.zeros(n, np.int64), r, nxt], 1), np.stack([r, 1 + n + np.arange(n), nxt], 1)]).astype(np.int32)
    perm = rng.permutation(len(f))                                       # the hub's entries arrive from all over the face list
    return v, C._colors(len(v), seed), f[perm]


def small_fans(valences=(31, 32, 33)):
    """Closed fans (:func:`hub_fan`) side by side: hubs with 2 x 31, 2 x 32 and 2 x 33 entries, around the 64 up to which the
    finishing kernel sorts a segment itself."""
    vs, cs, fs, n = [], [], [], 0
    for k, valence in enumerate(valences):
        v, c, f = hub_fan(valence, seed=10 + k)
        vs.append(v + np.float32(200.0 * k)), cs.append(c), fs.append(f + n)
        n += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(cs), np.concatenate(fs).astype(np.int32)


def repeated_corners(seed: int = 3):
    """12 vertices; faces (a, a, b), (a, b, a), (a, a, a) among ordinary ones, a duplicate face and a vertex in no face."""
    f = np.array([[0, 1, 2], [1, 1, 3], [4, 5, 4], [6, 6, 6], [0, 2, 3], [0, 1, 2], [7, 8, 9], [9, 8, 10], [2, 2, 2], [3, 1, 1]], np.int32)
    return C._positions(12, seed), C._colors(12, seed), f


def sparse_triangles():
    """mesh_clean_ref.isolated_triangles(70, n_vertices=100003): all boundary, most vertices isolated; the first isolated vertices
    get -0.0 and denormal coordinates, whose bits a copy must keep."""
    v, c, f = C.isolated_triangles(70, n_vertices=100003)
    v = v.copy()
    free = np.setdiff1d(np.arange(len(v)), f.reshape(-1))[:4]
    v[free[0]] = np.float32(-0.0)
    v[free[1]] = np.array([1e-45, -1e-45, 1e-40], np.float32)
    v[free[2]] = np.array([-0.0, 5e-39, 1.0], np.float32)
    return v, c, f


def strip_and_triangles():
    f, nv = C.strip_and_triangles(1 << 16, 10000)
    return C._positions(nv, 5), C._colors(nv, 5), f


def random_faces():
    return C._positions(500, 4), C._colors(500, 4), C.random_faces(500, 2000, seed=2)


def dense_faces():
    """600 random faces over 40 vertices: edges in three and more faces, repeated faces and corners, segments around the 64 entries
    up to which the finishing kernel sorts a segment itself."""
    return C._positions(40, 6), C._colors(40, 6), C.random_faces(40, 600, seed=3)
