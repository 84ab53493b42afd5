"""A numpy restatement of the component rule of DESIGN §1.11 (include/cds_mvsnet_hip.h, "Connected components of a triangle mesh
and the removal of the small ones"), and the meshes the tests of csrc/mesh_clean.hip share.  A plain union-find over the faces in
their order; no kernel, no torch."""
import functools

import numpy as np


def labels(faces: np.ndarray, n_vertices: int) -> np.ndarray:
    """Rules 1 and 2: label[v] = the smallest vertex index of v's component, int32 [V]."""
    parent = list(range(int(n_vertices)))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:                                        # path compression
            parent[x], x = r, parent[x]
        return r

    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)                    # the root of a tree is its smallest vertex
    return np.array([find(v) for v in range(int(n_vertices))], dtype=np.int32).reshape(int(n_vertices))


def components(faces: np.ndarray, n_vertices: int) -> dict:
    """Rules 1-3 -> {"label" int32 [V], "components" int32 [C] ascending, "faces" int64 [C]}."""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    lab = labels(faces, n_vertices)
    comps = np.nonzero(lab == np.arange(n_vertices))[0].astype(np.int32)
    per_vertex = np.bincount(lab[faces[:, 0]], minlength=max(int(n_vertices), 1)).astype(np.int64)   # a face counts for its first vertex
    return {"label": lab, "components": comps, "faces": per_vertex[comps]}


def select(counts: np.ndarray, min_faces: int = 0, keep_largest: int = 0) -> np.ndarray:
    """Rule 4 over the components in ascending label order -> bool [C]."""
    counts = np.asarray(counts, np.int64)
    keep = counts >= int(min_faces)
    if int(keep_largest) > 0:
        order = sorted(range(len(counts)), key=lambda i: (-int(counts[i]), i))     # count descending, label ascending
        first = np.zeros(len(counts), bool)
        first[order[:int(keep_largest)]] = True
        keep &= first
    return keep


def clean(vertices: np.ndarray, colors: np.ndarray, faces: np.ndarray, min_faces: int = 0, keep_largest: int = 0):
    """Rules 1-5 -> ({"vertices", "colors", "faces"}, info as mesh.clean_mesh's, without "rounds")."""
    vertices, colors = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(colors, np.uint8).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nv, nf = len(vertices), len(faces)
    c = components(faces, nv)
    kept = select(c["faces"], min_faces, keep_largest)
    kept_label = np.zeros(max(nv, 1), bool)
    kept_label[c["components"]] = kept
    fkeep = kept_label[c["label"][faces[:, 0]]] if nf else np.zeros(0, bool)
    vkeep = np.zeros(nv, bool)
    vkeep[faces[fkeep].reshape(-1)] = True
    new = np.cumsum(vkeep) - 1
    out = {"vertices": vertices[vkeep], "colors": colors[vkeep], "faces": new[faces[fkeep]].astype(np.int32).reshape(-1, 3)}
    info = {"components": (len(kept), int((kept & (c["faces"] > 0)).sum()) if nf else 0), "vertices": (nv, int(vkeep.sum())),
            "faces": (nf, int(fkeep.sum())), "largest": int(c["faces"].max()) if nf and len(kept) else 0}
    return out, info


# ---------------------------------------------------------------------------------------------------------------- meshes
TETRA = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)                    # the 4 faces of a tetrahedron


def _colors(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def sphere_with_debris():
    """The analytic sphere of mesh_ref (4568 faces, 2286 vertices, one component) and two translated tetrahedra after it:
    components 0, 2286 and 2290 with 4568, 4 and 4 faces.  -> (vertices, colors, faces); computed once, not to be modified."""
    import mesh_ref
    m = mesh_ref.analytic_case("sphere")[1]
    v, c, f = m["vertices"], m["colors"], m["faces"]
    n = len(v)
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    verts = np.concatenate([v, corner + np.float32(30.0), corner + np.float32(40.0)]).astype(np.float32)
    cols = np.concatenate([c, _colors(8, 1)])
    faces = np.concatenate([f, TETRA + n, TETRA + n + 4]).astype(np.int32)
    return verts, cols, faces


def two_fans():
    """Two fans of 3 triangles that share the vertex 3 and nothing else: one component of 6 faces over 9 vertices."""
    faces = np.array([[3, 0, 1], [3, 1, 2], [3, 2, 4], [3, 5, 6], [3, 6, 7], [3, 7, 8]], np.int32)
    return _positions(9, 2), _colors(9, 2), faces


def odd_faces():
    """10 vertices: a face with a repeated index (1, 1, 4) that still ties 1 to 4, a duplicate face, a face whose first vertex is
    not the smallest of its component, and the vertices 0 and 9 in no face.  Components 0 (0 faces), 1 (3: the faces that start
    at 1, 4, 4), 2 (2: the face and its duplicate), 9 (0)."""
    faces = np.array([[1, 1, 4], [2, 3, 5], [4, 6, 7], [2, 3, 5], [4, 7, 8]], np.int32)
    return _positions(10, 3), _colors(10, 3), faces


def _positions(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(100 + seed).normal(size=(n, 3)).astype(np.float32)


def isolated_triangles(n_faces: int, n_vertices=None, seed: int = 0):
    """n_faces triangles over 3 n_faces vertices of their own, at seeded random places among n_vertices >= 3 n_faces."""
    nv = 3 * n_faces if n_vertices is None else int(n_vertices)
    rng = np.random.default_rng(seed)
    where = np.sort(rng.choice(nv, 3 * n_faces, replace=False)) if nv > 3 * n_faces else np.arange(3 * n_faces)
    faces = rng.permutation(where).reshape(n_faces, 3).astype(np.int32)
    return _positions(nv, seed), _colors(nv, seed), faces


def strip(n_vertices: int, order: str = "ascending", seed: int = 0) -> np.ndarray:
    """The triangle strip (i, i + 1, i + 2) over n_vertices vertices, numbered along the strip ("ascending"), against it
    ("descending") or by a seeded permutation ("random") -> faces int32 [n_vertices - 2, 3]."""
    i = np.arange(n_vertices - 2, dtype=np.int64)
    faces = np.stack([i, i + 1, i + 2], 1)
    if order == "descending":
        faces = n_vertices - 1 - faces
    elif order == "random":
        faces = np.random.default_rng(seed).permutation(n_vertices)[faces]
    elif order != "ascending":
        raise ValueError(order)
    return faces.astype(np.int32)


def strip_and_triangles(n_strip: int = 1 << 16, n_triangles: int = 10000):
    """The ascending strip and n_triangles isolated triangles on vertices after it, interleaved in face order: the triangle j
    stands before the strip face j floor((n_strip - 2) / n_triangles) -> (faces, n_vertices)."""
    s = strip(n_strip)
    t = (n_strip + np.arange(3 * n_triangles, dtype=np.int64)).reshape(n_triangles, 3).astype(np.int32)
    at = np.arange(n_triangles, dtype=np.int64) * (len(s) // n_triangles)
    faces = np.insert(s, at, t, axis=0)
    return np.ascontiguousarray(faces, np.int32), n_strip + 3 * n_triangles


def random_faces(n_vertices: int, n_faces: int, seed: int) -> np.ndarray:
    """Seeded random index triples; collisions give faces with a repeated index."""
    return np.random.default_rng(seed).integers(0, n_vertices, (n_faces, 3)).astype(np.int32)
