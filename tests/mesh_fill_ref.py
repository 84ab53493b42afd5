"""The rule of csrc/mesh_fill.hip (rules 1-6 of include/cds_mvsnet_hip.h) restated in numpy: plain loops over a dict
of edges, and a walk without pruning.  Then the meshes that the CPU and the GPU tests of the rule share."""
import numpy as np

MAX_EDGES = 4096
CANONICAL_NAN = np.uint32(0x7fc00000)


def valid_faces(faces, nv):
    """Rule 1 -> bool [F]."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < nv)).all(1)
    return inside & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])


def borders(faces, nv):
    """Rules 1-3 -> {"next" int32 [V], -1 where the vertex is not regular, "regular" bool [V], "border_edges": int}."""
    held = {}                                                            # undirected edge -> the directed slots that hold it
    ok = valid_faces(faces, nv)
    for t, face in enumerate(np.asarray(faces).reshape(-1, 3).tolist()):
        if not ok[t]:
            continue
        for k in range(3):
            a, b = face[k], face[(k + 1) % 3]
            held.setdefault((min(a, b), max(a, b)), []).append((a, b))
    leave, enter, nxt = np.zeros(nv, np.int64), np.zeros(nv, np.int64), np.full(nv, -1, np.int32)
    count = 0
    for slots in held.values():
        if len(slots) != 1:
            continue
        a, b = slots[0]
        count += 1
        leave[a] += 1
        enter[b] += 1
        nxt[a] = b
    regular = (leave == 1) & (enter == 1)
    nxt[~regular] = -1
    return {"next": nxt, "regular": regular, "border_edges": count}


def loops(faces, nv, max_edges=None):
    """Rule 4 -> the loops as lists of vertices, v0 first, in ascending order of v0; with max_edges only those that are filled."""
    b = borders(faces, nv)
    nxt, regular = b["next"], b["regular"]
    seen = np.zeros(nv, bool)
    found = []
    for v0 in range(nv):
        if not regular[v0] or seen[v0]:
            continue
        path, v, closed = [], v0, False
        while regular[v] and not seen[v]:
            seen[v] = True
            path.append(int(v))
            v = int(nxt[v])
            if v == v0:
                closed = True
                break
        if closed:                                                       # v0 is the smallest: every smaller vertex was seen before
            found.append(path)
    if max_edges is not None:
        found = [p for p in found if 3 <= len(p) <= max_edges]
    return found, b["border_edges"]


def centre(vertices, colors, path):
    """Rule 5's new vertex of a loop of 4 or more edges -> (float32 [3], uint8 [3])."""
    n = len(path)
    pos = np.zeros(3, np.float32)
    with np.errstate(all="ignore"):
        for c in range(3):
            s = np.float64(0.0)
            for v in path:
                s = s + np.float64(vertices[v, c])
            m = s / np.float64(n)
            pos[c] = np.float32(m)
            if np.isnan(m):
                pos[c:c + 1].view(np.uint32)[0] = CANONICAL_NAN
    csum = [sum(int(colors[v, c]) for v in path) for c in range(3)]
    return pos, np.array([(2 * s + n) // (2 * n) for s in csum], np.uint8)


def fill(vertices, colors, faces, max_edges):
    """Rules 1-6 -> ({"vertices", "colors", "faces"}, info) as mesh.fill_holes."""
    if isinstance(max_edges, bool) or not isinstance(max_edges, (int, np.integer)) or not (3 <= max_edges <= MAX_EDGES):
        raise ValueError(f"max_edges must be an int in 3..{MAX_EDGES}, got {max_edges!r}")
    nv, nf = len(vertices), len(faces)
    filled, before = loops(faces, nv, max_edges) if nv and nf else ([], 0)
    new_v, new_c, new_f = [], [], []
    for path in filled:
        n = len(path)
        if n == 3:
            new_f.append([path[0], path[2], path[1]])
            continue
        c = nv + len(new_v)
        p, q = centre(vertices, colors, path)
        new_v.append(p)
        new_c.append(q)
        new_f.extend([path[(k + 1) % n], path[k], c] for k in range(n))
    out = {"vertices": np.concatenate([vertices, np.array(new_v, np.float32).reshape(-1, 3)]),
           "colors": np.concatenate([colors, np.array(new_c, np.uint8).reshape(-1, 3)]),
           "faces": np.concatenate([faces, np.array(new_f, np.int32).reshape(-1, 3)])}
    if new_v:                                                            # np.array of float32 rows keeps their bits
        out["vertices"][nv:].view(np.uint32)[:] = np.stack(new_v).view(np.uint32)
    closed = sum(len(p) for p in filled)
    info = {"max_edges": int(max_edges), "loops": len(filled), "largest": max([len(p) for p in filled], default=0),
            "border_edges": (before, before - closed), "vertices": (nv, nv + len(new_v)), "faces": (nf, nf + len(new_f))}
    return out, info


def border_count_by_unique(faces, nv):
    """A second border finder that shares nothing with :func:`borders`: np.unique over the sorted undirected keys of the valid
    faces -> (the number of edges held once, the sorted array of their (a, b) as directed)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)[valid_faces(faces, nv)]
    a, b = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
    key = np.minimum(a, b) * nv + np.maximum(a, b)
    uniq, first, counts = np.unique(key, return_index=True, return_counts=True)
    once = first[counts == 1]
    directed = np.stack([a[once], b[once]], 1)
    return int((counts == 1).sum()), directed[np.lexsort((directed[:, 1], directed[:, 0]))]


def signed_volume(vertices, faces):
    """Sum of the signed volumes of the tetrahedra (0, a, b, c), in fp64: the volume of a closed, outward-oriented mesh."""
    p = np.asarray(vertices, np.float64)[np.asarray(faces)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ------------------------------------------------------------------------------------------------------------------- meshes
def _colors(nv, seed):
    return np.random.default_rng(seed).integers(0, 256, (nv, 3)).astype(np.uint8)


def open_tetrahedron():
    """A tetrahedron, outward, without the face opposite vertex 0 -> (v, c, f)."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2]], np.int32)          # the missing one is (1, 2, 3)
    return v, _colors(4, 1), f


def cube(open_side=True):
    """The unit cube [0,1]^3 as 12 outward triangles; with open_side without the two of the side x = 1."""
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32)      # index = x + 2 y + 4 z
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]   # z=0, z=1, y=0, y=1, x=0, x=1
    if open_side:
        quads = quads[:5]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, _colors(8, 2), f


def lone_triangle():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 1]], np.float32)
    return v, _colors(3, 3), np.array([[0, 1, 2]], np.int32)


def grid(quads=12, seed=4):
    """A planar grid of quads x quads quads in z = 0.5, each cut into two triangles, counter-clockwise seen from +z."""
    n = quads + 1
    ys, xs = np.mgrid[0:n, 0:n]
    v = np.stack([xs.reshape(-1), ys.reshape(-1), np.full(n * n, 0.5)], 1).astype(np.float32)
    f = []
    for j in range(quads):
        for i in range(quads):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i
            f += [(a, b, c), (a, c, d)]
    return v, _colors(n * n, seed), np.array(f, np.int32)


def grow_hole(faces, nv, n, seed_face, allowed):
    """The faces of a disc-shaped patch whose rim has n edges: from seed_face, repeatedly the first face (in index order) that
    shares exactly one edge with the patch and whose third vertex is allowed and not yet on it, which adds one edge to the rim and
    keeps the rim a simple cycle -> the sorted face indices."""
    faces = np.asarray(faces)
    patch, used, edges = [seed_face], set(faces[seed_face].tolist()), set()
    for k in range(3):
        edges.add(frozenset((int(faces[seed_face][k]), int(faces[seed_face][(k + 1) % 3]))))
    assert all(allowed[x] for x in used)
    while len(patch) + 2 < n:
        for t in range(len(faces)):
            if t in patch:
                continue
            tri = faces[t].tolist()
            inside = [x for x in tri if x in used]
            if len(inside) != 2 or frozenset(inside) not in edges:
                continue
            new = [x for x in tri if x not in used][0]
            if not allowed[new]:
                continue
            patch.append(t)
            used.add(new)
            edges.update(frozenset((new, x)) for x in inside)
            break
        else:
            raise AssertionError(f"the patch stopped growing at {len(patch) + 2} edges")
    return sorted(patch)


def grid_with_hole(n, quads=12, also=()):
    """The grid with one hole of n >= 3 edges that touches the grid's rim nowhere, and without the faces ``also`` -> (v, c, f)."""
    v, c, f = grid(quads)
    m = quads + 1
    ij = np.arange(m * m)
    interior = ((ij % m) > 0) & ((ij % m) < quads) & ((ij // m) > 0) & ((ij // m) < quads)
    gone = grow_hole(f, len(v), n, 2 * (quads + 1), interior)
    return v, c, np.delete(f, gone + list(also), axis=0)


def renumber(v, c, f, new_of_old):
    """The same mesh with vertex old stored at row new_of_old[old]."""
    new_of_old = np.asarray(new_of_old)
    order = np.argsort(new_of_old)
    return v[order], c[order], new_of_old[f].astype(np.int32)


def loop_of(f, nv, n):
    """The one loop of n edges of a mesh."""
    (path,) = [p for p in loops(f, nv)[0] if len(p) == n]
    return path


def renumbered_loop(mesh, n, place, descending=False, seed=5):
    """mesh has one loop of n edges.  A random renumbering of all vertices under which the labels of that loop's vertices ascend
    along ``next`` (descend with ``descending``), the smallest at position ``place`` of the loop as it was."""
    v, c, f = mesh
    path = loop_of(f, len(v), n)
    perm = np.random.default_rng(seed).permutation(len(v))
    labels = np.sort(perm[path])
    for k in range(n):
        at = (place + k) % n if not descending else (place - k) % n
        perm[path[at]] = labels[k]
    return renumber(v, c, f, perm)


def ring_strip(around=10000, rows=3, hole=0):
    """A ring-shaped strip of rows x around quads: two rims of ``around`` edges each.  hole: 0, or the edge count (3..around) of
    a hole punched into the middle row as a run of hole - 2 triangles."""
    ring = np.arange(around)
    ang = 2.0 * np.pi * ring / around
    v = np.concatenate([np.stack([(10.0 + r) * np.cos(ang), (10.0 + r) * np.sin(ang), np.zeros(around)], 1) for r in range(rows + 1)])
    f = []
    for r in range(rows):
        a, b = r * around + ring, r * around + (ring + 1) % around
        d, e = a + around, b + around
        f.append(np.stack([np.stack([a, b, e], 1), np.stack([a, e, d], 1)], 1).reshape(-1, 3))
    f = np.concatenate(f).astype(np.int32)
    if hole:
        assert rows >= 3
        inner = np.zeros(len(v), bool)
        inner[around:rows * around] = True
        f = np.delete(f, grow_hole(f, len(v), hole, (rows // 2) * 2 * around + 2 * (around // 3), inner), axis=0)
    return v.astype(np.float32), _colors(len(v), 6), f


def patches(count, seed=7):
    """``count`` separate patches of 3 x 3 quads, the middle quad missing: a hole of 4 edges and a rim of 12 each.  The vertices of
    all patches are interleaved in memory by a random permutation, and so are the faces."""
    v0, c0, f0 = grid(3)
    f0 = np.delete(f0, [8, 9], axis=0)
    nv = len(v0)
    v = np.concatenate([v0 + np.array([5.0 * k, 0, 0], np.float32) for k in range(count)])
    f = np.concatenate([f0 + nv * k for k in range(count)]).astype(np.int32)
    rng = np.random.default_rng(seed)
    v, c, f = renumber(v, _colors(len(v), seed), f, rng.permutation(len(v)))
    return v, c, f[rng.permutation(len(f))]


def bow_tie():
    """The grid with two one-quad holes that share the vertex between them."""
    v, c, f = grid(6)
    q = lambda i, j: [2 * (j * 6 + i), 2 * (j * 6 + i) + 1]
    return v, c, np.delete(f, q(2, 2) + q(3, 3), axis=0)


def fin():
    """The grid with a one-quad hole, and a triangle standing on one of the grid's inner edges: that edge is held three times."""
    v, c, f = grid(6)
    f = np.delete(f, [2 * (2 * 6 + 2), 2 * (2 * 6 + 2) + 1], axis=0)
    v = np.concatenate([v, np.array([[4.5, 4.0, 1.5]], np.float32)])
    c = np.concatenate([c, np.array([[9, 9, 9]], np.uint8)])
    return v, c, np.concatenate([f, np.array([[4 * 7 + 4, 4 * 7 + 5, len(v) - 1]], np.int32)])


def flipped():
    """The grid with a one-quad hole and, elsewhere, one face whose winding is reversed: its three edges are held twice in the
    same direction."""
    v, c, f = grid(6)
    turned = 2 * (4 * 6 + 3)
    f[turned] = f[turned][::-1]
    return v, c, np.delete(f, [2 * (2 * 6 + 2), 2 * (2 * 6 + 2) + 1], axis=0)


def with_degenerate_faces():
    """The grid with a 5-edge hole, and faces (a, a, b), (a, b, a) and (a, a, a) appended and inserted."""
    v, c, f = grid_with_hole(5, 6)
    extra = np.array([[3, 3, 9], [10, 17, 10], [5, 5, 5]], np.int32)
    return v, c, np.insert(f, [0, 20, len(f)], extra, axis=0)


def odd_bits():
    """A hole of 6 edges whose rim carries -0.0, denormals, an infinity and a NaN (one special kind per coordinate and vertex), a
    hole of 4 whose rim is all -0.0 in z, and rim colours whose means fall on .5 exactly."""
    q = 2 * (8 * 12 + 8)
    v, c, f = grid_with_hole(6, 12, also=(q, q + 1))
    path = loop_of(f, len(v), 6)
    v[path[0], 2] = -0.0
    v[path[1], 2] = np.float32(1e-40)
    v[path[2], 2] = np.float32(-3e-45)
    v[path[3], 0] = np.inf
    v[path[4], 1] = np.nan
    for k, p in enumerate(path):
        c[p] = (k % 2, 200 + (k < 3), 255)                               # means 0.5, 200.5 and 255
    second = loop_of(f, len(v), 4)
    v[second, 2] = -0.0
    c[second] = [[1, 2, 3], [2, 2, 3], [1, 3, 3], [2, 3, 4]]             # means 1.5, 2.5 and 3.25
    return v, c, f


def random_faces(nv=60, nf=150, seed=8):
    """Random faces over few vertices: edges held once, twice either way and more often, repeated corners."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, nv, (nf, 3)).astype(np.int32)
    v = rng.normal(size=(nv, 3)).astype(np.float32)
    return v, _colors(nv, seed), f


def random_punched_grid(seed, quads=10, holes=14):
    """The grid with random faces deleted: holes that merge, touch in a vertex and reach the rim."""
    v, c, f = grid(quads, seed)
    rng = np.random.default_rng(seed)
    return v, c, np.delete(f, rng.choice(len(f), holes, replace=False), axis=0)
