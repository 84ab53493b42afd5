"""Float32 numpy restatement of the gipuma-style fusion rule (cds_mvsnet_amd/gipuma.py, csrc/gipuma.hip).

Sequential over the reference views, vectorised over the pixels of one view.  The steps are those of the issue that defines
the feature ("Add gipuma-style depth-map fusion on the GPU", section "The rule to implement"), numbered as there.  Every
operation below is one float32 operation in the order the kernel's header comment records, so the GPU result must be
bitwise equal to this one.
"""
import numpy as np

F32 = np.float32


def constants(cams):
    """Step 2: per view P [3,4], Minv [3,3] (float32 of float64) and fb [V,V] (float32)."""
    P32, M32, centres, f = [], [], [], []
    for cam in cams:
        cam = np.asarray(cam, np.float32)
        k4 = np.zeros((4, 4))
        k4[:3, :3] = cam[1, :3, :3]
        P = np.matmul(k4, cam[0])[:3]                   # what mvsnet_to_gipuma_cam writes
        minv = np.linalg.inv(P[:, :3])
        centres.append(-minv @ P[:, 3])
        P32.append(P.astype(np.float32))
        M32.append(minv.astype(np.float32))
        f.append(np.float64(cam[1, 0, 0]))
    c = np.stack(centres)
    fb = np.asarray(f)[:, None] * np.linalg.norm(c[:, None, :] - c[None, :, :], axis=-1)
    return P32, M32, fb.astype(np.float32)


def _row3(m, q0, q1, q2):
    return (m[0] * q0 + m[1] * q1) + m[2] * q2


def _row4(m, q0, q1, q2):
    return ((m[0] * q0 + m[1] * q1) + m[2] * q2) + m[3]


def prob_filter(depth, conf, prob_threshold):
    """Step 1: depth [h,w], conf [3,h,w] -> D'."""
    keep = np.ones(depth.shape, bool)
    for k in range(3):
        keep &= conf[k] > F32(prob_threshold[k])
    return np.where(keep, depth, F32(0)).astype(np.float32)


def fuse(depths, confs, cams, images, prob_threshold=(0.0, 0.0, 0.0), disp_threshold=0.2, num_consistent=3,
         depth_min=0.001, depth_max=100000.0):
    """depths: V arrays [h,w]; confs: V arrays [3,h,w]; cams: V arrays [2,4,4]; images: V arrays [h,w,3] uint8.
    -> {"points" [N,3] float32, "colors" [N,3] uint8, "ref_view" [N], "used" [V,h,w] bool}."""
    V = len(depths)
    h, w = np.asarray(depths[0]).shape
    for v in range(V):
        if np.asarray(depths[v]).shape != (h, w) or np.asarray(confs[v]).shape != (3, h, w) or \
                np.asarray(images[v]).shape != (h, w, 3):
            raise ValueError(f"view {v} does not have the size of view 0 ({h}x{w})")
    D = [prob_filter(np.asarray(depths[v], np.float32), np.asarray(confs[v], np.float32), prob_threshold) for v in range(V)]
    img = [np.asarray(images[v]).astype(np.int64) for v in range(V)]
    P, M, fb = constants(cams)
    dmin, dmax, disp = F32(depth_min), F32(depth_max), F32(disp_threshold)
    used = np.zeros((V, h, w), bool)
    xs = np.tile(np.arange(w), h)
    ys = np.repeat(np.arange(h), w)
    pts, cols, refs = [], [], []
    with np.errstate(all="ignore"):
        for r in range(V):                                                   # step 3: r ascending, one after another
            d = D[r].reshape(-1)
            act = ~used[r].reshape(-1) & (d > dmin) & (d < dmax)
            pix = np.nonzero(act)[0]
            d, x, y = d[pix], xs[pix].astype(np.float32), ys[pix].astype(np.float32)
            Pr, Mr = P[r], M[r]
            q0, q1, q2 = d * x - Pr[0, 3], d * y - Pr[1, 3], d - Pr[2, 3]
            X0, X1, X2 = _row3(Mr[0], q0, q1, q2), _row3(Mr[1], q0, q1, q2), _row3(Mr[2], q0, q1, q2)
            S0, S1, S2 = X0.copy(), X1.copy(), X2.copy()
            rgb = img[r][ys[pix], xs[pix]].copy()
            n = np.zeros(pix.size, np.int64)
            marks = []
            for j in range(V):
                if j == r:
                    continue
                Pj, Mj, f = P[j], M[j], fb[r, j]
                a, b, z = _row4(Pj[0], X0, X1, X2), _row4(Pj[1], X0, X1, X2), _row4(Pj[2], X0, X1, X2)
                ok = z > 0
                u, v = a / z, b / z
                ok &= (u >= 0) & (u < F32(w)) & (v >= 0) & (v < F32(h))
                fu = np.where(ok, np.minimum(np.floor(u + F32(0.5)), F32(w - 1)), F32(0)).astype(np.float32)
                fv = np.where(ok, np.minimum(np.floor(v + F32(0.5)), F32(h - 1)), F32(0)).astype(np.float32)
                iu, iv = fu.astype(np.int64), fv.astype(np.int64)
                dj = D[j][iv, iu]
                ok &= (dj > dmin) & (dj < dmax)
                ok &= np.abs(f / z - f / dj) < disp
                e0, e1, e2 = dj * fu - Pj[0, 3], dj * fv - Pj[1, 3], dj - Pj[2, 3]
                S0 = np.where(ok, S0 + _row3(Mj[0], e0, e1, e2), S0)
                S1 = np.where(ok, S1 + _row3(Mj[1], e0, e1, e2), S1)
                S2 = np.where(ok, S2 + _row3(Mj[2], e0, e1, e2), S2)
                rgb += np.where(ok[:, None], img[j][iv, iu], 0)
                n += ok
                marks.append((j, ok, iu, iv))
            emit = n >= num_consistent
            for j, ok, iu, iv in marks:
                sel = ok & emit
                used[j, iv[sel], iu[sel]] = True
            k = (n[emit] + 1).astype(np.float32)
            pts.append(np.stack([S0[emit] / k, S1[emit] / k, S2[emit] / k], 1).astype(np.float32))
            cols.append((rgb[emit] // (n[emit] + 1)[:, None]).astype(np.uint8))
            refs.append(np.full(int(emit.sum()), r, np.int32))
    return {"points": np.concatenate(pts) if pts else np.zeros((0, 3), np.float32),
            "colors": np.concatenate(cols) if cols else np.zeros((0, 3), np.uint8),
            "ref_view": np.concatenate(refs) if refs else np.zeros(0, np.int32), "used": used}
