"""Seeded synthetic inputs for tests, fixtures and bench.py.

No dataset exists on the build / GPU boxes, so every workload is generated here: DTU-like cameras
(finite epipoles, ~90 % in-image samples), images in [0,1), per-pair feature maps in (-1,1) and
jittered per-pixel depth hypotheses.  Everything is created on CPU from explicit seeds so the same
numbers are obtained in the build container (where the fixtures are captured from the reference)
and on the GPU box.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

Tensor = torch.Tensor


def _rot_xy(a: float, b: float) -> np.ndarray:
    rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    return rx @ ry


def make_cameras(n_views: int, H: int, W: int, refine: bool = False, seed: int = 0,
                 baseline: Tuple[float, float, float] = (40.0, 15.0, 10.0)) -> Dict[str, Tensor]:
    """Multi-scale projection dict as the reference's datasets build it (general_eval.py:167-200):
    ``stageK`` -> [1,N,2,4,4] with [:, :, 0] = world-to-camera extrinsic and [:, :, 1, :3, :3] = intrinsic
    scaled per stage (refine=False: K/4, K/2, K; refine=True adds stage4 = K and halves the others).
    View 0 is the reference camera (identity extrinsic)."""
    rs = np.random.RandomState(seed)
    K = np.array([[0.9 * W, 0, W / 2.0], [0, 0.9 * W, H / 2.0], [0, 0, 1.0]])
    ext = []
    for i in range(n_views):
        E = np.eye(4)
        if i > 0:
            a, b = rs.uniform(-0.06, 0.06, 2)
            t = rs.uniform(-1, 1, 3) * np.array(baseline)
            t[2] += 5.0 if i % 2 else -5.0
            E[:3, :3] = _rot_xy(a, b)
            E[:3, 3] = t
        ext.append(E)
    names = ["stage1", "stage2", "stage3"] + (["stage4"] if refine else [])
    divs = [8.0, 4.0, 2.0, 1.0] if refine else [4.0, 2.0, 1.0]
    out = {}
    for name, dv in zip(names, divs):
        mats = np.zeros((1, n_views, 2, 4, 4), dtype=np.float32)
        for i in range(n_views):
            mats[0, i, 0] = ext[i]
            Ks = K.copy()
            Ks[:2] /= dv
            mats[0, i, 1, :3, :3] = Ks
        out[name] = torch.from_numpy(mats)
    return out


def stage_cameras(n_views: int, h: int, w: int, seed: int = 0) -> Tensor:
    """[1,N,2,4,4] cameras whose intrinsics address an h x w grid directly (single-stage workloads)."""
    return make_cameras(n_views, h, w, refine=False, seed=seed)["stage3"]


def make_depth_values(n: int = 192, start: float = 425.0, step: float = 2.5) -> Tensor:
    return (start + step * torch.arange(n, dtype=torch.float32)).unsqueeze(0)


def make_images(n_views: int, H: int, W: int, seed: int = 0, smooth: bool = True) -> Tensor:
    """[1,N,3,H,W] in [0,1): bicubic-upsampled low-resolution noise plus fine noise (image-like spectrum)."""
    g = torch.Generator().manual_seed(seed)
    if not smooth:
        return torch.rand(1, n_views, 3, H, W, generator=g)
    low = torch.rand(n_views, 3, max(2, H // 16), max(2, W // 16), generator=g)
    img = F.interpolate(low, (H, W), mode="bicubic", align_corners=False)
    img = 0.8 * img + 0.2 * torch.rand(n_views, 3, H, W, generator=g)
    return img.clamp(0.0, 0.999).unsqueeze(0).contiguous()


def _boxblur5(x: Tensor) -> Tensor:
    c = x.shape[1]
    k = torch.full((c, 1, 5, 5), 1.0 / 25.0)
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode="replicate"), k, groups=c)


def make_pair_features(n_src: int, C: int, h: int, w: int, seed: int = 1,
                       sharp: bool = False) -> List[Dict[str, Tuple[Tensor, Tensor, Tensor]]]:
    """Per-pair stage features in the reference's layout: list over source views of
    {'ref': (fea [1,C,h,w], nc_sum [1,1,h,w], |nc| [1,1,h,w]), 'src': (...)} with fea in (-1,1).
    sharp=False: 5x5 box-blurred (smooth, image-feature like); sharp=True: white tanh noise (large
    correlation dynamic range and maximal sensitivity to the sampling position)."""
    g = torch.Generator().manual_seed(seed)
    feats = []
    for _ in range(n_src):
        d = {}
        for key in ("ref", "src"):
            fea = torch.tanh(torch.randn(1, C, h, w, generator=g) * (1.5 if sharp else 1.0))
            if not sharp:
                fea = _boxblur5(fea)
            nc_sum = torch.rand(1, 1, h, w, generator=g)
            nc = torch.rand(1, 1, h, w, generator=g)
            d[key] = (fea.contiguous(), nc_sum, nc)
        feats.append(d)
    return feats


def make_hypotheses(D: int, h: int, w: int, lo: float = 425.0, hi: float = 902.5, jitter: float = 3.0,
                    seed: int = 1) -> Tensor:
    """[1,D,h,w] planes linspace(lo,hi,D) plus a per-pixel uniform jitter."""
    g = torch.Generator().manual_seed(seed + 1000)
    planes = torch.linspace(lo, hi, D).view(1, D, 1, 1)
    return (planes + jitter * torch.rand(1, D, h, w, generator=g)).contiguous()


def make_fusion_scene(n_views: int, h: int, w: int, seed: int = 0, outlier_frac: float = 0.15,
                      pixel_offset: float = 0.5) -> Dict[str, Tensor]:
    """Geometrically consistent depth maps for the filtering / fusion step: every camera of ``make_cameras`` looks at
    the height field Z = 650 + 40 sin(X/60) cos(Y/50) (world = reference-camera frame); per-view depth = camera-frame z of
    the ray/surface intersection (fixed-point iteration in float64) through image point (x + pixel_offset, y + pixel_offset)
    of pixel (x, y) (0.0: gipuma's convention, integer pixel coordinates).  A fraction of the pixels gets a ±(2..6)% depth
    error so that the geometric masks are mixed; confidences are uniform in [0,1).
    -> depths [N,h,w], confs [N,3,h,w], cams [N,2,4,4] (intrinsic [3,3] = 1), imgs [N,h,w,3]."""
    cams = make_cameras(n_views, h, w, refine=False, seed=seed)["stage3"][0].clone()
    cams[:, 1, 3, 3] = 1.0
    rs = np.random.RandomState(seed + 77)
    ys, xs = np.meshgrid(np.arange(h) + pixel_offset, np.arange(w) + pixel_offset, indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], 0).reshape(3, -1)
    depths = []
    for i in range(n_views):
        E = cams[i, 0].double().numpy()
        K = cams[i, 1, :3, :3].double().numpy()
        R, t = E[:3, :3], E[:3, 3:4]
        d = np.linalg.inv(K) @ pix                         # camera-frame rays with z = 1
        rd, rt = R.T @ d, R.T @ t
        lam = np.full(pix.shape[1], 650.0)
        for _ in range(20):
            P = rd * lam - rt
            surf = 650.0 + 40.0 * np.sin(P[0] / 60.0) * np.cos(P[1] / 50.0)
            lam = (surf + rt[2]) / rd[2]
        dep = lam.reshape(h, w)
        bad = rs.rand(h, w) < outlier_frac
        dep = np.where(bad, dep * (1.0 + rs.choice([-1.0, 1.0], (h, w)) * rs.uniform(0.02, 0.06, (h, w))), dep)
        depths.append(dep.astype(np.float32))
    g = torch.Generator().manual_seed(seed + 5)
    return {"depths": torch.from_numpy(np.stack(depths)), "confs": torch.rand(n_views, 3, h, w, generator=g),
            "cams": cams.contiguous(), "imgs": torch.rand(n_views, h, w, 3, generator=g)}


def fusion_surface(x, y):
    """The height field of :func:`make_fusion_scene`: Z = 650 + 40 sin(X/60) cos(Y/50) (float64 numpy)."""
    return 650.0 + 40.0 * np.sin(np.asarray(x, np.float64) / 60.0) * np.cos(np.asarray(y, np.float64) / 50.0)


def make_dtu_scene(half_x: float, half_y: float, spacing: float, res: float, margin: float, plane_z: float = 630.0,
                   n_pred: int = 0, noise: float = 0.0, outlier_frac: float = 0.0, outlier_range: float = 30.0,
                   holes: int = 0, hole_radius: float = 0.0, seed: int = 0) -> Dict[str, np.ndarray]:
    """Ground truth in the layout of the DTU evaluation files for the height field of :func:`make_fusion_scene`, over
    |X| <= half_x, |Y| <= half_y:
      stl      float32 [N,3]: the surface sampled on a jittered grid of pitch ``spacing``;
      ObsMask  bool [X,Y,Z] voxels of side ``res`` over BB: set within ``margin`` of the surface, except for |X| > 0.8 half_x;
      BB       float64 [2,3] (min row, max row), Res, P float64 [4]: the plane z = plane_z (points above it count);
      pred     float32 [n_pred,3] (when n_pred > 0): uniform surface samples with N(0, noise) normal jitter, ``holes`` empty
               discs of radius ``hole_radius`` and ``outlier_frac`` points moved up to ``outlier_range`` off the surface."""
    rs = np.random.RandomState(seed)
    xs = np.arange(-half_x, half_x + 1e-9, spacing)
    ys = np.arange(-half_y, half_y + 1e-9, spacing)
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    gx = gx.reshape(-1) + rs.uniform(-0.25, 0.25, gx.size) * spacing
    gy = gy.reshape(-1) + rs.uniform(-0.25, 0.25, gy.size) * spacing
    stl = np.stack([gx, gy, fusion_surface(gx, gy)], 1).astype(np.float32)
    lo = np.array([-half_x, -half_y, 610.0]) - margin - 2 * res
    hi = np.array([half_x, half_y, 690.0]) + margin + 2 * res
    bb = np.stack([lo, hi])
    dims = np.floor((hi - lo) / res).astype(int) + 1
    cx, cy, cz = [lo[a] + res * np.arange(dims[a]) for a in range(3)]          # voxel (i,j,k) centre: BB(1,:) + (ijk - 1) Res
    surf = fusion_surface(cx[:, None], cy[None, :])
    obs = np.abs(cz[None, None, :] - surf[:, :, None]) <= margin
    obs[np.abs(cx) > 0.8 * half_x] = False
    out = {"stl": stl, "ObsMask": obs, "BB": bb, "Res": float(res), "P": np.array([0.0, 0.0, 1.0, -plane_z])}
    if n_pred > 0:
        g = torch.Generator().manual_seed(seed + 1)
        u = torch.rand(n_pred, 2, generator=g, dtype=torch.float64).numpy()
        px, py = (u[:, 0] * 2 - 1) * half_x, (u[:, 1] * 2 - 1) * half_y
        pz = fusion_surface(px, py) + noise * torch.randn(n_pred, generator=g, dtype=torch.float64).numpy()
        pred = np.stack([px, py, pz], 1)
        if holes:
            centres = rs.uniform(-0.7, 0.7, (holes, 2)) * np.array([half_x, half_y])
            inside = np.zeros(pred.shape[0], bool)
            for c in centres:
                inside |= ((pred[:, 0] - c[0]) ** 2 + (pred[:, 1] - c[1]) ** 2) <= hole_radius ** 2
            pred = pred[~inside]
        n_out = int(outlier_frac * pred.shape[0])
        if n_out:
            idx = rs.choice(pred.shape[0], n_out, replace=False)
            pred[idx] += rs.uniform(-outlier_range, outlier_range, (n_out, 3))
        out["pred"] = pred.astype(np.float32)
    return out


def tt_surface(x, y, half: float, centre=(1.5, -0.8, 0.6)):
    """The height field of :func:`make_tt_scene` over |x - cx|, |y - cy| <= half (float64 numpy)."""
    u = (np.asarray(x, np.float64) - centre[0]) / half
    v = (np.asarray(y, np.float64) - centre[1]) / half
    return centre[2] + half * (0.25 * np.sin(3.0 * u) * np.cos(2.0 * v) + 0.08 * np.sin(7.0 * u + 1.0) * np.sin(5.0 * v))


def similarity(deg: float, axis, shift, scale: float = 1.0, about=(0.0, 0.0, 0.0)) -> np.ndarray:
    """4x4 float64: scale times a rotation of ``deg`` degrees about ``axis`` through the point ``about``, then ``shift``."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = math.radians(deg)
    R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    c = np.asarray(about, np.float64)
    out = np.eye(4)
    out[:3, :3] = scale * R
    out[:3, 3] = c - scale * (R @ c) + np.asarray(shift, np.float64)
    return out


def make_tt_scene(n_gt: int = 30_000, n_pred: int = 30_000, tau: float = 0.01, density: float = 2.0, noise: float = 0.4,
                  outlier_frac: float = 0.04, outlier_range: float = 8.0, holes: int = 4, hole_radius: float = 10.0,
                  misalign=(0.15, 1.2, 1.002), seed: int = 0) -> Dict[str, object]:
    """A scene in the layout of a Tanks and Temples training scene, sized by ``tau`` (noise, outlier_range, hole_radius and
    the misalignment's shift are in units of tau):
      gt      float32 [~n_gt,3]: the surface :func:`tt_surface` on a jittered grid with ``density`` points per tau;
      crop    a concave (notched L) polygon volume orthogonal to Z that cuts both clouds (the keys of tt_eval.read_crop);
      trans   float64 [4,4]: the scene's nominal alignment, prediction frame -> ground-truth frame (a rigid motion);
      true_trans  ``D @ trans`` with D the small similarity ``misalign`` = (degrees, shift in tau, scale) about the centre;
      pred    float32 [<= n_pred,3]: uniform random surface samples (another sampling than gt) with N(0, noise tau) height
              noise, ``holes`` empty discs and ``outlier_frac`` points moved up to ``outlier_range`` tau away, mapped into
              the prediction frame by the inverse of true_trans: ``trans`` alone leaves it misaligned by D;
      tau."""
    rs = np.random.RandomState(seed)
    centre = np.array([1.5, -0.8, 0.6])
    side = max(int(round(math.sqrt(n_gt))), 2)
    spacing = tau / density
    half = 0.5 * (side - 1) * spacing
    g = (np.arange(side) - 0.5 * (side - 1)) * spacing
    gx, gy = np.meshgrid(g, g, indexing="ij")
    gx = centre[0] + gx.reshape(-1) + rs.uniform(-0.3, 0.3, gx.size) * spacing
    gy = centre[1] + gy.reshape(-1) + rs.uniform(-0.3, 0.3, gy.size) * spacing
    gt = np.stack([gx, gy, tt_surface(gx, gy, half, centre)], 1).astype(np.float32)

    px = centre[0] + rs.uniform(-1.0, 1.0, n_pred) * half
    py = centre[1] + rs.uniform(-1.0, 1.0, n_pred) * half
    pred = np.stack([px, py, tt_surface(px, py, half, centre) + rs.randn(n_pred) * noise * tau], 1)
    if holes:
        hc = centre[:2] + rs.uniform(-0.7, 0.7, (holes, 2)) * half
        gone = np.zeros(n_pred, bool)
        for c in hc:
            gone |= ((pred[:, 0] - c[0]) ** 2 + (pred[:, 1] - c[1]) ** 2) <= (hole_radius * tau) ** 2
        pred = pred[~gone]
    n_out = int(outlier_frac * len(pred))
    if n_out:
        idx = rs.choice(len(pred), n_out, replace=False)
        pred[idx] += rs.uniform(-outlier_range, outlier_range, (n_out, 3)) * tau

    # a notched L in units of half around the centre: concave, and it leaves a band of both clouds outside
    shape = np.array([[-0.9, -0.85], [0.88, -0.9], [0.9, -0.1], [0.35, -0.05], [0.2, 0.3], [0.3, 0.92], [-0.5, 0.88],
                      [-0.45, 0.35], [-0.92, 0.3]])
    poly = np.concatenate([centre[:2] + shape * half, np.zeros((len(shape), 1))], 1)
    crop = {"orthogonal_axis": "Z", "axis_min": float(centre[2] - 0.24 * half), "axis_max": float(centre[2] + 0.3 * half),
            "bounding_polygon": poly}

    trans = similarity(25.0, (0.2, -0.1, 1.0), (0.3, -0.2, 0.1))
    D = similarity(misalign[0], (1.0, 0.6, 0.8), np.array([0.5, -0.3, 0.8]) / math.sqrt(0.98) * misalign[1] * tau, misalign[2], centre)
    true_trans = D @ trans
    inv = np.linalg.inv(true_trans)
    pred = (pred @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return {"gt": gt, "pred": pred, "crop": crop, "trans": trans, "true_trans": true_trans, "tau": float(tau)}


def _min_track_angle(centres: np.ndarray, xyz: np.ndarray, pt: np.ndarray, img: np.ndarray) -> float:
    """Smallest angle (degrees) at a point between two camera centres that both observe it, over all tracks."""
    N, P = len(centres), len(xyz)
    key = np.unique(pt.astype(np.int64) * N + img)
    p, i = key // N, key % N
    L = np.bincount(p, minlength=P)
    start = np.concatenate([[0], np.cumsum(L)])
    best = 180.0
    for length in np.unique(L[L >= 2]):
        pts = np.nonzero(L == length)[0]
        a, b = np.triu_indices(int(length), 1)
        chunk = max(1, 1_000_000 // len(a))
        for c in range(0, len(pts), chunk):
            q = pts[c:c + chunk]
            im = i[start[q][:, None] + np.arange(length)]
            u = centres[im[:, a]] - xyz[q][:, None, :]
            v = centres[im[:, b]] - xyz[q][:, None, :]
            cos = (u * v).sum(-1) / np.linalg.norm(u, axis=-1) / np.linalg.norm(v, axis=-1)
            best = min(best, float(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))).min()))
    return best


def make_colmap_model(n_images: int, n_points: int, seed: int = 0, mean_track: float = 6.0, long_frac: float = 0.01,
                      n_isolated: int = 2, invalid_frac: float = 0.02, dup_frac: float = 0.0, min_angle_deg=0.1,
                      width: int = 96, height: int = 64, ext: str = ".jpg", decimals=None):
    """A COLMAP sparse model (cameras, images, Points3D of ``cds_mvsnet_amd.colmap``) for the converter's tests and timings:
    ``n_images`` cameras on an arc of radius 20 (with some height jitter) look at a slab of ``n_points`` points around the origin.

    * Visibility: every point is seen by a window of consecutive cameras.  Its length is 2 + Poisson for most points and
      uniform in [2, n_images] for a fraction ``long_frac`` (so track lengths range from 2 to all images), with a mean near
      ``mean_track``.  The last ``n_isolated`` cameras of the arc are almost isolated: they see three points each.
    * COLMAP image ids and point ids are ascending with gaps; the ``images`` dict is filled in a shuffled order.
    * ``invalid_frac`` of every image's observations (at least two) carry point id -1; ``dup_frac`` of the valid observations
      are repeated in the same image (same point id, not in the track).
    * Two cameras, PINHOLE (id 1) and SIMPLE_RADIAL (id 3), alternate over the images.
    * ``decimals``: round the point coordinates to this many decimals (shorter text models for fixtures).
    * ``min_angle_deg``: asserts that every pair of cameras sharing a point subtends at least this angle at it (None skips
      the check, which visits every term of the pair score)."""
    from .colmap import Camera, Image, Points3D
    rs = np.random.RandomState(seed)
    N, P = int(n_images), int(n_points)
    n_iso = min(int(n_isolated), max(0, N - 2))
    M = N - n_iso                                           # cameras that take part in the windows
    # ---- cameras ----
    span = np.radians(min(300.0, max(90.0, 0.5 * N)))
    phi = np.linspace(-span / 2, span / 2, N) + rs.uniform(-0.2, 0.2, N) * span / max(N - 1, 1)
    centres = np.stack([20.0 * np.sin(phi), rs.uniform(-1.5, 1.5, N), -20.0 * np.cos(phi)], 1)
    qvecs, tvecs = np.zeros((N, 4)), np.zeros((N, 3))
    rots = np.zeros((N, 3, 3))
    for i in range(N):
        z = -centres[i] / np.linalg.norm(centres[i])
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])                # rows: camera axes in the world
        tr = np.trace(R)                                    # > -1 here: the cameras stay near upright
        w = 0.5 * math.sqrt(max(1e-12, 1.0 + tr))
        q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
        qvecs[i] = q / np.linalg.norm(q)
        from .colmap import rotation_matrix
        rots[i] = rotation_matrix(qvecs[i])
        tvecs[i] = -rots[i] @ centres[i]
    centres = -np.einsum("nji,nj->ni", rots, tvecs)         # the centres the poses really have
    f = 0.9 * width
    cameras = {1: Camera(1, "PINHOLE", width, height, np.array([f, f * 1.01, width / 2.0, height / 2.0])),
               3: Camera(3, "SIMPLE_RADIAL", width, height, np.array([f * 0.98, width / 2.0 + 0.5, height / 2.0 - 0.5, 0.01]))}
    cam_of = np.where(np.arange(N) % 2 == 0, 1, 3)
    image_ids = np.cumsum(rs.randint(1, 4, N)) + 2
    # ---- points and tracks ----
    xyz = rs.uniform(-1.0, 1.0, (P, 3)) * np.array([4.0, 2.0, 0.5])
    if decimals is not None:
        xyz = np.round(xyz, decimals)
    point_ids = np.cumsum(rs.randint(1, 4, P)).astype(np.int64) + 10
    lam = max(0.5, mean_track - 2.0 - long_frac * M / 2.0)
    L = 2 + rs.poisson(lam, P)
    long_ = rs.rand(P) < long_frac
    L[long_] = rs.randint(2, M + 1, int(long_.sum()))
    if P:
        L[rs.randint(P)] = M                                # at least one track through every camera of the arc
    L = np.minimum(L, M)
    first = (rs.rand(P) * (M - L + 1)).astype(np.int64)
    pt = np.repeat(np.arange(P), L)
    img = np.repeat(first - np.concatenate([[0], np.cumsum(L)[:-1]]), L) + np.arange(L.sum())
    if n_iso:
        pt = np.concatenate([pt, rs.randint(0, P, 3 * n_iso)])
        img = np.concatenate([img, np.repeat(np.arange(M, N), 3)])
        key = np.unique(pt.astype(np.int64) * N + img)
        pt, img = key // N, key % N
    if min_angle_deg is not None:
        got = _min_track_angle(centres, xyz, pt, img)
        assert got >= min_angle_deg, f"make_colmap_model: smallest triangulation angle {got} < {min_angle_deg} degrees"
    # ---- observations: tracked, duplicated, invalid; shuffled inside every image ----
    E0 = pt.size
    dup = rs.choice(E0, int(dup_frac * E0), replace=False) if dup_frac > 0 else np.zeros(0, np.int64)
    n_inv = np.maximum(2, (invalid_frac * np.bincount(img, minlength=N)).astype(np.int64)) if invalid_frac > 0 else \
        np.zeros(N, np.int64)
    o_pt = np.concatenate([pt, pt[dup], np.full(int(n_inv.sum()), -1)])
    o_img = np.concatenate([img, img[dup], np.repeat(np.arange(N), n_inv)])
    tracked = np.concatenate([np.ones(E0, bool), np.zeros(o_pt.size - E0, bool)])
    perm = rs.permutation(o_pt.size)
    perm = perm[np.argsort(o_img[perm], kind="stable")]
    o_pt, o_img, tracked = o_pt[perm], o_img[perm], tracked[perm]
    iptr = np.concatenate([[0], np.cumsum(np.bincount(o_img, minlength=N))])
    idx2d = np.arange(o_pt.size) - iptr[o_img]
    X = xyz[np.maximum(o_pt, 0)]
    cam = np.einsum("eij,ej->ei", rots[o_img], X) + tvecs[o_img]
    K = np.stack([np.array([[c.params[0], c.params[1 if c.model == "PINHOLE" else 0]],
                            [c.params[2 if c.model == "PINHOLE" else 1], c.params[3 if c.model == "PINHOLE" else 2]]])
                  for c in (cameras[k] for k in cam_of)])               # [N, (f, c), (x, y)]
    xy = K[o_img, 0] * cam[:, :2] / cam[:, 2:3] + K[o_img, 1] + rs.normal(0, 0.3, (o_pt.size, 2))
    xy[o_pt < 0] = rs.uniform(0, 1, (int((o_pt < 0).sum()), 2)) * np.array([width, height])
    xy = np.round(xy, 2 if decimals is None else min(2, decimals))
    images = {}
    for i in rs.permutation(N):
        s, e = iptr[i], iptr[i + 1]
        ids = np.where(o_pt[s:e] >= 0, point_ids[np.maximum(o_pt[s:e], 0)], -1).astype(np.int64)
        images[int(image_ids[i])] = Image(int(image_ids[i]), qvecs[i].copy(), tvecs[i].copy(), int(cam_of[i]),
                                          "img_%04d%s" % (i, ext), xy[s:e].copy(), ids)
    t = np.nonzero(tracked)[0]
    t = t[np.argsort(o_pt[t], kind="stable")]
    tptr = np.concatenate([[0], np.cumsum(np.bincount(o_pt[t], minlength=P))])
    points = Points3D(point_ids, xyz, rs.randint(0, 256, (P, 3)), np.round(rs.uniform(0.1, 2.0, P), 3), tptr,
                      image_ids[o_img[t]], idx2d[t])
    return cameras, images, points
