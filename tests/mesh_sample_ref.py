"""Numpy restatement of the surface sampling rule (the rule is stated in include/cds_mvsnet_hip.h), the yardstick
of csrc/mesh_sample.hip.  Vectorised over the samples; every decision in float64 or integers, every float64 expression bracketed as
the rule writes it.  Imports nothing from the package."""
import numpy as np

MAX_N = 1 << 15


def _spans(n, spacing, l2):
    """Rule 1's test: ((double)n spacing) ((double)n spacing) >= L2."""
    s = n.astype(np.float64) * np.float64(spacing)
    return s * s >= l2


def counts(vertices: np.ndarray, faces: np.ndarray, spacing: float) -> np.ndarray:
    """Rule 1 -> n int64 [F]: 0 for a face with a corner that is not finite, else the smallest n >= 1 that passes the test,
    clamped to MAX_N + 1."""
    f = np.asarray(faces).reshape(-1, 3)
    p = np.asarray(vertices, np.float32).astype(np.float64)[f]              # [F, 3 corners, 3]
    finite = np.isfinite(p).all((1, 2))
    p = np.where(finite[:, None, None], p, 0.0)

    def edge2(a, b):
        d = a - b
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    l2 = np.maximum(np.maximum(edge2(p[:, 1], p[:, 0]), edge2(p[:, 2], p[:, 1])), edge2(p[:, 0], p[:, 2]))
    with np.errstate(over="ignore", invalid="ignore"):
        guess = np.ceil(np.sqrt(l2) / np.float64(spacing))
    n = np.clip(np.nan_to_num(guess, nan=1.0, posinf=MAX_N + 1.0), 1, MAX_N + 1).astype(np.int64)
    while True:                                                              # downwards, then upwards: the test decides, not the guess
        down = (n > 1) & _spans(n - 1, spacing, l2)
        if not down.any():
            break
        n[down] -= 1
    while True:
        up = (n <= MAX_N) & ~_spans(n, spacing, l2)
        if not up.any():
            break
        n[up] += 1
    return np.where(finite, n, 0)


def weights(n, k):
    """Rule 2's integer weights of sample k of a face with subdivision n (arrays or scalars) -> (wa, wb, wc), int64."""
    n, k = np.asarray(n, np.int64), np.asarray(k, np.int64)
    r = np.floor(np.sqrt(k.astype(np.float64))).astype(np.int64)
    r = r - (r * r > k)
    r = r + ((r + 1) * (r + 1) <= k)
    assert ((r * r <= k) & (k < (r + 1) * (r + 1))).all()
    c = k - r * r
    j = c >> 1
    odd = (c & 1) == 1
    p = np.where(odd, 3 * r + 1, 3 * r + 2)
    q = np.where(odd, 3 * j + 2, 3 * j + 1)
    return 3 * n - p, p - q, q


def sample(vertices: np.ndarray, colors: np.ndarray, faces: np.ndarray, spacing: float):
    """-> ({"points" float32 [N,3], "colors" uint8 [N,3], "face" int32 [N]}, {"faces", "points", "max_n", "skipped"}, n int64 [F]).
    ValueError for a spacing that is not finite and > 0 and for a face with n > MAX_N."""
    spacing = float(spacing)
    if not (spacing > 0 and np.isfinite(spacing)):
        raise ValueError(f"spacing must be positive, got {spacing}")
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    col = np.asarray(colors, np.uint8).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    n = counts(v, f, spacing)
    max_n = int(n.max()) if len(n) else 0
    if max_n > MAX_N:
        raise ValueError(f"a face needs more than {MAX_N} subdivisions at spacing {spacing}")
    n2 = n * n
    total = int(n2.sum())
    face = np.repeat(np.arange(len(f), dtype=np.int64), n2)
    k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(n2) - n2, n2)
    nn = n[face]
    wa, wb, wc = weights(nn, k)
    assert total == 0 or (min(wa.min(), wb.min(), wc.min()) > 0 and (wa + wb + wc == 3 * nn).all())
    corner = f[face].astype(np.int64)                                        # [N, 3]
    points = np.empty((total, 3), np.float32)
    d3n = (3 * nn).astype(np.float64)
    fa, fb, fc = wa.astype(np.float64), wb.astype(np.float64), wc.astype(np.float64)
    v64 = v.astype(np.float64)
    for c in range(3):
        a, b, cc = v64[corner[:, 0], c], v64[corner[:, 1], c], v64[corner[:, 2], c]
        points[:, c] = (((fa * a + fb * b) + fc * cc) / d3n).astype(np.float32)
    ci = col.astype(np.int64)
    out_col = np.empty((total, 3), np.uint8)
    for c in range(3):
        s = wa * ci[corner[:, 0], c] + wb * ci[corner[:, 1], c] + wc * ci[corner[:, 2], c]
        out_col[:, c] = ((2 * s + 3 * nn) // (6 * nn)).astype(np.uint8)
    info = {"faces": int(len(f)), "points": total, "max_n": max_n, "skipped": int((n == 0).sum())}
    return {"points": points, "colors": out_col, "face": face.astype(np.int32)}, info, n


# ----------------------------------------------------------------------------------------------------------------- meshes
def cube(side: float = 4.0):
    """The 12-face cube [0, side]^3, outward winding; corner colours from the corner's bits."""
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32) * np.float32(side)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    c = np.array([[255 * (i & 1), 255 * ((i >> 1) & 1), 255 * ((i >> 2) & 1)] for i in range(8)], np.uint8)
    return v, c, f


def small_faces_around_a_large_one(n_small: int = 1000, spacing: float = 1.0, n_large: int = 300, seed: int = 5):
    """n_small faces with edges below ``spacing`` (n = 1) and, in the middle of the list, one face whose longest edge asks for
    n = n_large."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-50, 50, (n_small, 1, 3))
    tri = base + rng.uniform(-0.25, 0.25, (n_small, 3, 3)) * spacing
    big = np.array([[0, 0, 0], [(n_large - 0.5) * spacing, 0, 0], [0.5 * n_large * spacing, 0.66 * n_large * spacing, 3.0]], np.float64)
    v = np.concatenate([tri.reshape(-1, 3), big]).astype(np.float32)
    f = np.arange(3 * n_small, dtype=np.int32).reshape(n_small, 3)
    f = np.insert(f, n_small // 2, np.array([3 * n_small, 3 * n_small + 1, 3 * n_small + 2], np.int32), axis=0)
    c = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    return v, c, np.ascontiguousarray(f, np.int32)


def height_field_mesh(xs, ys, height):
    """A triangulated height field over the grid xs x ys (two faces per cell) -> (vertices float32 [len(xs) len(ys), 3], faces)."""
    gx, gy = np.meshgrid(np.asarray(xs, np.float64), np.asarray(ys, np.float64))
    v = np.stack([gx, gy, height(gx, gy)], -1).reshape(-1, 3).astype(np.float32)
    w, faces = len(xs), []
    for y in range(len(ys) - 1):
        for x in range(w - 1):
            a, b, c, d = y * w + x, y * w + x + 1, (y + 1) * w + x + 1, (y + 1) * w + x
            faces += [(a, b, c), (a, c, d)]
    return v, np.array(faces, np.int32)
