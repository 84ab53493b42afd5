"""The numpy restatement of the seam-levelling rule (rules L1-L6 of include/cds_mvsnet_hip.h) on top of texture_ref:
plain loops in the order the rule states, fp64 with its bracketing, decisions in integers.  numpy does one IEEE operation per
ufunc call and never contracts, so the GPU kernels are expected to agree bit for bit in everything but the offsets of rule L3,
which a linear solver produces.  Also the seam jump, the exposure helper and the plane set-up the tests measure the feature on."""
import functools

import numpy as np

import render_ref as R
import texture_ref as T

RIDGE = 2.0 ** -10
OMEGA = 0.75


# ------------------------------------------------------------------------------------------------------------------ the rule
def nodes(faces, view, n_views):
    """Rule L1 -> (node_key int64 [N], corner_node int32 [NF,3], corners: per node the ascending list of its corner indices)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    keys = {}
    for face in range(len(f)):
        if view[face] >= 0:
            for k in range(3):
                keys.setdefault(int(f[face, k]) * n_views + int(view[face]), []).append(3 * face + k)
    node_key = np.array(sorted(keys), np.int64)
    rank = {key: n for n, key in enumerate(node_key.tolist())}
    corner_node = np.full((len(f), 3), -1, np.int32)
    for key, cs in keys.items():
        for c in cs:
            corner_node[c // 3, c % 3] = rank[key]
    return node_key, corner_node, [sorted(keys[key]) for key in node_key.tolist()]


def bilinear(img, u, v):
    """The image branch of rule 6 at the pixel coordinates u, v [N] of one image [h,w,3] -> the unrounded fp64 values [N,3]."""
    h, w = img.shape[:2]
    x = np.minimum(np.maximum(u, 0.5), w - 0.5) - 0.5
    y = np.minimum(np.maximum(v, 0.5), h - 0.5) - 0.5
    xl, yl = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    xh, yh = np.minimum(xl + 1, w - 1), np.minimum(yl + 1, h - 1)
    fx, fy = x - xl, y - yl
    gx, gy = 1.0 - fx, 1.0 - fy
    im = img.astype(np.float64)
    return np.stack([(((gx * gy) * im[yl, xl, ch] + (fx * gy) * im[yl, xh, ch]) + (gx * fy) * im[yh, xl, ch]) + (fx * fy) * im[yh, xh, ch]
                     for ch in range(3)], 1)


def samples(vertices, images, cams, node_key, n_views):
    """Rule L2 -> (sample fp64 [N,3], ok uint8 [N])."""
    V = np.asarray(vertices, np.float32).astype(np.float64)
    s, ok = np.zeros((len(node_key), 3), np.float64), np.zeros(len(node_key), np.uint8)
    for n, key in enumerate(node_key.tolist()):
        vertex, label = key // n_views, key % n_views
        u, v, z = T._project(cams[label], V[vertex][None])
        if z[0] > 0 and np.isfinite(u[0]) and np.isfinite(v[0]):
            s[n], ok[n] = bilinear(images[label], u, v)[0], 1
    return s, ok


def vertex_groups(node_key, n_views):
    """The nodes of every vertex, ascending -> a list of lists."""
    groups = {}
    for n, key in enumerate(node_key.tolist()):
        groups.setdefault(key // n_views, []).append(n)
    return [groups[k] for k in sorted(groups)]


def pair_table(sample, ok, node_key, n_views):
    """Rule L3 -> int64 [V,V,4]: cnt, dsum[3]."""
    q = np.floor(sample * 256.0 + 0.5).astype(np.int64)
    table = np.zeros((n_views, n_views, 4), np.int64)
    for group in vertex_groups(node_key, n_views):
        for x, i in enumerate(group):
            for j in group[x + 1:]:
                if ok[i] and ok[j]:
                    a, b = int(node_key[i]) % n_views, int(node_key[j]) % n_views
                    table[a, b, 0] += 1
                    table[a, b, 1:] += q[i] - q[j]
    return table


def offsets(table, node_key, n_views):
    """Rule L3: the normal equations of the energy, entry by entry, solved per channel -> o fp64 [V,3]."""
    n_label = np.bincount(node_key % n_views, minlength=n_views) if len(node_key) else np.zeros(n_views, np.int64)
    A, rhs = np.zeros((n_views, n_views), np.float64), np.zeros((n_views, 3), np.float64)
    for a in range(n_views):
        A[a, a] += RIDGE * max(int(n_label[a]), 1)
        for b in range(a + 1, n_views):
            cnt = float(table[a, b, 0])
            if cnt:
                D = table[a, b, 1:].astype(np.float64) / (256.0 * cnt)
                A[a, a] += cnt; A[b, b] += cnt; A[a, b] -= cnt; A[b, a] -= cnt
                rhs[a] -= cnt * D
                rhs[b] += cnt * D
    return np.stack([np.linalg.solve(A, rhs[:, ch]) for ch in range(3)], 1)


def offsets_lstsq(table, node_key, n_views):
    """Rule L3 stated independently: one row per term of the energy, numpy.linalg.lstsq -> (o fp64 [V,3], the matrix of the rows)."""
    n_label = np.bincount(node_key % n_views, minlength=n_views) if len(node_key) else np.zeros(n_views, np.int64)
    rows, right = [], []
    for a in range(n_views):
        for b in range(a + 1, n_views):
            if table[a, b, 0]:
                r = np.zeros(n_views)
                w = np.sqrt(float(table[a, b, 0]))
                r[a], r[b] = w, -w
                rows.append(r)
                right.append(-w * table[a, b, 1:].astype(np.float64) / (256.0 * float(table[a, b, 0])))
    for a in range(n_views):
        r = np.zeros(n_views)
        r[a] = np.sqrt(RIDGE * max(int(n_label[a]), 1))
        rows.append(r)
        right.append(np.zeros(3))
    M = np.array(rows)
    return np.linalg.lstsq(M, np.array(right), rcond=None)[0], M


def step(sample, ok, groups_of, corners, corner_node, g, lam):
    """Rule L5: one iteration -> the next g.  groups_of[n]: the nodes of n's vertex, ascending."""
    out = np.empty_like(g)
    lam = np.float64(lam)
    for n in range(len(g)):
        S, T_, c, d = np.zeros(3), np.zeros(3), 0, 0
        if ok[n]:
            for m in groups_of[n]:
                if m != n and ok[m]:
                    S = S + ((sample[m] + g[m]) - sample[n])
                    c += 1
        for corner in corners[n]:
            f, k = corner // 3, corner % 3
            for m in (corner_node[f, (k + 1) % 3], corner_node[f, (k + 2) % 3]):
                T_ = T_ + g[m]
                d += 1
        den = np.float64(c) + lam * np.float64(d)
        out[n] = g[n] + OMEGA * (((S + lam * T_) / den) - g[n])
    return out


def iterate(lv, o, iters, lam, keep):
    """Rules L4 and L5 from the tables of :func:`level` and the offsets o -> {iteration: g} for the iterations of ``keep``."""
    node_key, V = lv["node_key"], len(o)
    g = np.asarray(o, np.float64)[node_key % V] if len(node_key) else np.zeros((0, 3))
    groups_of = {}
    for group in vertex_groups(node_key, V):
        for n in group:
            groups_of[n] = group
    g_at = {0: g.copy()} if 0 in keep else {}
    for it in range(1, iters + 1):
        g = step(lv["sample"], lv["ok"], groups_of, lv["corners"], lv["corner_node"], g, lam)
        if it in keep:
            g_at[it] = g.copy()
    return g_at


def fill_level(vertices, colors, faces, images, cams, view, c, origin, H, W, corner_node, g):
    """Rule 6 with rule L6 on its image branch -> atlas uint8 [H,W,3]."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    atlas = T.fill(vertices, colors, f, images, cams, view, c, origin, H, W)       # the vertex-colour branch and unseen faces
    face, i, j, P = T.texel_points(vertices, f, c)
    cc = np.asarray(c, np.int64)
    den = (cc[face] - 2).astype(np.float64)
    wb = ((i.astype(np.float64) + 0.5) - 1.0) / den
    wc = ((j.astype(np.float64) + 0.5) - 1.0) / den
    wa = (1.0 - wb) - wc
    N = len(g)
    with np.errstate(all="ignore"):
        for v in np.unique(view[view >= 0]):
            cn = corner_node[face].astype(np.int64)
            sel = np.nonzero((view[face] == v) & ((cn >= 0) & (cn < N)).all(1))[0]
            u, vv, z = T._project(cams[v], P[sel])
            keep = (z > 0) & np.isfinite(u) & np.isfinite(vv)
            sel, u, vv = sel[keep], u[keep], vv[keep]
            val = bilinear(images[v], u, vv)
            cn = cn[sel]
            for ch in range(3):
                corr = (wa[sel] * g[cn[:, 0], ch] + wb[sel] * g[cn[:, 1], ch]) + wc[sel] * g[cn[:, 2], ch]
                t = val[:, ch] + corr
                t = np.where(t > 0, np.where(t < 255, t, 255.0), 0.0)
                atlas[origin[face[sel], 1] + j[sel], origin[face[sel], 0] + i[sel], ch] = np.floor(t + 0.5).astype(np.uint8)
    return atlas


def level(vertices, colors, faces, images, cams, iters, lam=0.1, scale=1.0, max_cell=256, min_px=1, base=None, force_offsets=None,
          keep=()):
    """Rules 1-6 and L1-L6 -> texture_ref.texture's dict plus "level": {"node_key", "corner_node", "sample", "ok", "offsets", "g",
    "table", "corners", "g_at": {iteration: g} for the iterations of ``keep``}.  base: the unlevelled result, when it is at hand;
    force_offsets: an o to use in the place of rule L3's (the library's own, or zeros)."""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    base = dict(base if base is not None else T.texture(vertices, colors, f, images, cams, scale, max_cell, min_px))
    if isinstance(images, (list, tuple)):
        images, cams = [a for img in images for a in img], np.concatenate(list(cams))
    V = len(cams)
    view = base["view"]
    node_key, corner_node, corners = nodes(f, view, V)
    s, ok = samples(vertices, images, cams, node_key, V)
    table = pair_table(s, ok, node_key, V)
    o = offsets(table, node_key, V) if force_offsets is None else np.asarray(force_offsets, np.float64)
    lv = {"node_key": node_key, "corner_node": corner_node, "sample": s, "ok": ok, "offsets": o, "table": table, "corners": corners}
    lv["g_at"] = iterate(lv, o, iters, lam, tuple(keep) + (iters,))
    g = lv["g"] = lv["g_at"][iters]
    cell = base["cell"]
    H, W = base["atlas"].shape[:2]
    base["atlas"] = fill_level(vertices, colors, f, images, cams, view, cell[:, 2], cell[:, :2], H, W, corner_node, g)
    base["level"] = lv
    return base


def seam_jump(sample, ok, node_key, n_views, g):
    """-> (pairs, the mean over the ok pairs of one vertex and the channels of |(s_i + g_i) - (s_j + g_j)|)."""
    total, pairs = 0.0, 0
    for group in vertex_groups(node_key, n_views):
        for x, i in enumerate(group):
            for j in group[x + 1:]:
                if ok[i] and ok[j]:
                    total += float(np.abs((sample[i] + g[i]) - (sample[j] + g[j])).sum())
                    pairs += 1
    return pairs, (total / (3 * pairs) if pairs else 0.0)


# ------------------------------------------------------------------------------------------------------------------ builders
def expose(img, gain=1.0, off=0.0):
    """An image under another exposure: floor(clip(gain img + off, 0, 255) + 0.5)."""
    return np.floor(np.clip(gain * img.astype(np.float64) + off, 0, 255) + 0.5).astype(np.uint8)


def two_faces(labels):
    """Two faces that share the edge (1, 2), and their view labels."""
    return np.array([(0, 1, 2), (2, 1, 3)], np.int32), np.array(labels, np.int32)


@functools.lru_cache(maxsize=None)
def plane_setup(n=9, n_views=3, offs=(0.0, 25.0, -20.0)):
    """The set-up the feature is measured on: plane_mesh(n) reversed, view_cameras at twice the resolution (128 x 96), the analytic
    pattern of texture_ref in every view -> (vertices, colours, faces, images, the same images under the offsets, cams)."""
    v, f = R.plane_mesh(n)
    f = np.ascontiguousarray(T.reversed_faces(f), np.int32)
    cams = R.view_cameras(n_views).copy()
    cams[:, 1, :2, :3] *= 2.0
    images = T.plane_images(cams, 96, 128)
    vc = np.floor(np.clip(T.pattern(v.astype(np.float64)), 0, 255) + 0.5).astype(np.uint8)
    shifted = np.stack([expose(img, 1.0, o) for img, o in zip(images, offs)])
    return v, vc, f, images, shifted, cams


def pattern_rms(vertices, faces, out, n=24):
    """The rms error of an atlas against the analytic pattern over a barycentric lattice of surface points, read back at their UVs,
    with the mean difference of every channel removed (a texture is as good under a constant exposure)."""
    V64 = np.asarray(vertices, np.float64)
    pts, uvs = [], []
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    keep = i + j < n - 1
    wb, wc = (i[keep] + 0.33) / n, (j[keep] + 0.33) / n
    wa = 1.0 - wb - wc
    for k, (a, b, c) in enumerate(faces):
        pts.append(wa[:, None] * V64[a] + wb[:, None] * V64[b] + wc[:, None] * V64[c])
        uv = out["uv"][k].astype(np.float64)
        uvs.append(wa[:, None] * uv[0] + wb[:, None] * uv[1] + wc[:, None] * uv[2])
    diff = T.atlas_lookup(out["atlas"], np.concatenate(uvs)) - T.pattern(np.concatenate(pts))
    diff = diff - diff.mean(0)
    return float(np.sqrt((diff ** 2).mean()))


@functools.lru_cache(maxsize=None)
def reference(name, n_views, iters, h=R.H, w=R.W, scale=1.0, max_cell=256, keep=()):
    """The restatement's levelled outputs for a named case of texture_ref; computed once, not to be modified."""
    v, c, f, images, cams = T.case(name, n_views, h, w)
    return level(v, c, f, images, cams, iters, scale=scale, max_cell=max_cell, base=T.reference(name, n_views, h, w, scale, max_cell),
                 keep=keep)
